"""ctypes binding of libmwengine.so (include/mwengine.h) — the only way the Python package
reaches the GPU.  There is deliberately NO CPU fallback: if the HIP library is missing or no
MI355X is visible, construction fails loudly.

The binding passes raw device pointers (``tensor.data_ptr()``) and the current HIP stream;
torch is used for memory and streams only.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys

import numpy as np

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
# (MW_ENGINE_LIB: a variant build of the library for A/B measurements — tools/perf; the product is csrc/libmwengine.so)
PRODUCT_PATH = os.path.join(_CSRC, "libmwengine.so")
LIB_PATH = os.environ.get("MW_ENGINE_LIB") or PRODUCT_PATH

ABI_VERSION = 4
MAX_REPEAT = 256            # MW_MAX_REPEAT
MAX_PLAN = MAX_REPEAT        # MW_MAX_PLAN
MAX_STACK = 16              # MW_MAX_STACK
STACK_PAD_RESET, STACK_PAD_ZERO = 0, 1
SNAPF_DEPTH, SNAPF_STACK = 1, 2     # MW_SNAPF_*
ENT_NONE, ENT_BOX, ENT_MESH, ENT_FRAME = 0, 1, 2, 3
POLY_ENTITY = 0x100          # mw_poly.nv flag: quad of a static entity, not a room
POLY_XF = 0x200              # ... drawn under its own glTranslatef / glRotatef (mw_poly.xf)
POLY_QUAD = 0x400            # ... issued inside glBegin(GL_QUADS) (walls, frames); otherwise GL_POLYGON
TASK_NONE, TASK_GOTO, TASK_PICKUP, TASK_PUTNEXT, TASK_SIDEWALK, TASK_SIGN, TASK_COLLECT = 0, 1, 2, 3, 4, 5, 6
GEN_NONE, GEN_HALLWAY, GEN_ONEROOM, GEN_PICKUP, GEN_MAZE, GEN_PROGRAM = 0, 1, 2, 3, 4, 5
OP_COIN, OP_DRAW_DIR, OP_PLACE, OP_FIXED, OP_BOX_SIZE, OP_COLOR, OP_APPEND = 1, 2, 3, 4, 5, 6, 7
PROG_MAX_ROOMS, PROG_MAX_TEX, PROG_MAX_OPS, PROG_MAX_ENTS = 16, 8, 48, 64
AUTORESET_OFF, AUTORESET_SAME_STEP, AUTORESET_NEXT_STEP = 0, 1, 2
OBS_HWC_U8, OBS_CWH_U8, OBS_GREY_F64 = 0, 1, 2
RNG_PHILOX, RNG_PCG64 = 0, 1
PATH_TILE, PATH_QUAD, PATH_QUAD_MESH, PATH_GENERIC = 0, 1, 2, 3

class MwRange(C.Structure):
    _fields_ = [("default", C.c_double), ("lo", C.c_double), ("hi", C.c_double)]

    @classmethod
    def of(cls, default, lo=None, hi=None):
        return cls(float(default), float(default if lo is None else lo), float(default if hi is None else hi))


class MwConfig(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32), ("device_id", C.c_int32), ("num_envs", C.c_int32),
        ("obs_width", C.c_int32), ("obs_height", C.c_int32), ("msaa", C.c_int32),
        ("max_ents", C.c_int32), ("max_polys", C.c_int32), ("max_segs", C.c_int32),
        ("max_visible", C.c_int32), ("shared_geometry", C.c_int32), ("task", C.c_int32),
        ("goal_ent", C.c_int32), ("goal_ent2", C.c_int32), ("num_objs", C.c_int32), ("max_episode_steps", C.c_int32),
        ("domain_rand", C.c_int32), ("generator", C.c_int32), ("autoreset", C.c_int32),
        ("agent_radius", C.c_double), ("agent_height", C.c_double), ("max_forward_step", C.c_double),
        ("forward_step", MwRange), ("forward_drift", MwRange), ("turn_step", MwRange),
        ("sky_color", MwRange * 3), ("light_pos", MwRange * 3), ("light_color", MwRange * 3),
        ("light_ambient", MwRange * 3), ("obj_color_bias", MwRange * 3),
        ("cam_height", MwRange), ("cam_fwd_disp", MwRange), ("cam_pitch", MwRange), ("cam_fov_y", MwRange),
        ("gen_args", C.c_double * 8),
        ("gen_tab", C.c_double * 12),
        ("gen_colors", C.c_double * 18),
        ("tex_nvar", C.c_int32 * 3), ("tex_var_id", (C.c_int32 * 9) * 3),
        ("tex_var_scale", ((C.c_double * 2) * 9) * 3),
        ("room_wall_height", C.c_double), ("room_no_ceiling", C.c_int32), ("rng_mode", C.c_int32),
    ]


class MwPoly(C.Structure):
    _fields_ = [("v", C.c_float * 12), ("uv", C.c_float * 8), ("n", C.c_float * 3),
                ("nv", C.c_int32), ("tex", C.c_int32), ("rgb", C.c_float * 3), ("xf", C.c_float * 4)]


POLY_DTYPE = np.dtype([("v", np.float32, (4, 3)), ("uv", np.float32, (4, 2)), ("n", np.float32, (3,)),
                       ("nv", np.int32), ("tex", np.int32), ("rgb", np.float32, (3,)), ("xf", np.float32, (4,))])
assert POLY_DTYPE.itemsize == C.sizeof(MwPoly) == 128


class MwProgRoom(C.Structure):
    _fields_ = [("nverts", C.c_int32), ("wall_tex", C.c_int32), ("floor_tex", C.c_int32), ("ceil_tex", C.c_int32),
                ("ox", C.c_double * 4), ("oz", C.c_double * 4), ("nx", C.c_double * 4), ("nz", C.c_double * 4),
                ("min_x", C.c_double), ("max_x", C.c_double), ("min_z", C.c_double), ("max_z", C.c_double), ("cdf", C.c_double)]


class MwProgOp(C.Structure):
    _fields_ = [("op", C.c_int32), ("slot", C.c_int32), ("room", C.c_int32), ("cond", C.c_int32), ("dir_mode", C.c_int32),
                ("flags", C.c_int32), ("lx", C.c_double), ("hx", C.c_double), ("lz", C.c_double), ("hz", C.c_double),
                ("dir", C.c_double), ("a", C.c_double), ("b", C.c_double)]


class MwGenProgram(C.Structure):
    _fields_ = [("n_rooms", C.c_int32), ("n_tex", C.c_int32), ("n_ops", C.c_int32), ("n_ents", C.c_int32),
                ("rooms", MwProgRoom * PROG_MAX_ROOMS),
                ("tex_nvar", C.c_int32 * PROG_MAX_TEX), ("tex_var_id", (C.c_int32 * 9) * PROG_MAX_TEX),
                ("tex_var_scale", ((C.c_double * 2) * 9) * PROG_MAX_TEX),
                ("ops", MwProgOp * PROG_MAX_OPS),
                ("ent_kind", C.c_int32 * PROG_MAX_ENTS), ("ent_mesh", C.c_int32 * PROG_MAX_ENTS), ("ent_static", C.c_int32 * PROG_MAX_ENTS),
                ("ent_pos", (C.c_double * 3) * PROG_MAX_ENTS), ("ent_dir", C.c_double * PROG_MAX_ENTS),
                ("ent_geom", (C.c_double * 9) * PROG_MAX_ENTS),
                ("colors", (C.c_double * 3) * 6), ("extent", C.c_double * 4), ("street", C.c_double * 4),
                ("sign_n", C.c_int32), ("pad", C.c_int32), ("sign_slot", C.c_int32 * 8), ("sign_reward", C.c_double * 8)]


class MwStateView(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in (
        "agent_pos", "agent_dir", "cam", "light", "carrying", "step_count", "num_picked_up",
        "ent_kind", "ent_mesh", "ent_static", "ent_pos", "ent_dir", "ent_geom", "extent")]


NAV_ENTITIES, NAV_JACOBI, NAV_GRID = 1, 2, 4     # MW_NAV_* flags
NAV_BLOCKED, NAV_UNREACHED = 0xFFFF, 0xFFFE
NAV_MAX_CELLS = 32768                   # MW_NAV_MAX_CELLS
NAV_MAX_INFLATE = 16                    # MW_NAV_MAX_INFLATE: mw_nav_build_grid's largest inflation radius in cells


class MwNavParams(C.Structure):
    _fields_ = [("cell", C.c_double), ("margin", C.c_double), ("reach", C.c_double), ("gx", C.c_int32), ("gz", C.c_int32),
                ("flags", C.c_int32), ("target_slot", C.c_int32)]


RAY_ENTITIES = 1                        # MW_RAY_ENTITIES
RAY_ENT = 0x10000                       # MW_RAY_ENT: hit = RAY_ENT + slot for an entity
RAY_MAX = 4096                          # MW_RAY_MAX


class MwRayParams(C.Structure):
    _fields_ = [("max_t", C.c_double), ("radius", C.c_double), ("rays", C.c_int32), ("flags", C.c_int32)]


SEEN_ENTITIES = 1                       # MW_SEEN_ENTITIES
SIGHT_MAX_VIEWS = 256                   # MW_SIGHT_MAX_VIEWS: mw_grid_sight's viewpoints per env and call
REGION_MAX = 256                        # MW_REGION_MAX: mw_grid_regions' listed regions per env and call (== SIGHT_MAX_VIEWS)

EGO_ENTITIES, EGO_NORTH = 1, 2          # MW_EGO_* flags
EGO_WALL, EGO_ENTITY, EGO_VISIBLE = 1, 2, 4     # MW_EGO_* planes
EGO_MAX_SIZE = 128                      # MW_EGO_MAX_SIZE

DEPTH_MAX_PIXELS = 65535                # MW_DEPTH_MAX_PIXELS
DEPTH_MAX_CELLS = 16384                 # the cells of a depth window or map: 4 bytes of LDS each (csrc/mw_depth.h)

LABELMAP_MAX_CELLS = 16384              # the cells of an object window or map: a key of LDS each (csrc/mw_labelmap.h)
LABELMAP_MAX_IDS = 255                  # the ids of an object map's per-object outputs; an id is 0 .. 254, a byte 1 + id

LABEL_NOTHING, LABEL_FLOOR, LABEL_CEILING, LABEL_WALL, LABEL_FRAME, LABEL_BOX, LABEL_MESH = range(7)       # MW_LABEL_* classes
LABEL_MESH_EXACT, LABEL_MESH_BOUNDS, LABEL_UNPRUNED = 0, 1, 2           # MW_LABEL_* flags


class MwLabelParams(C.Structure):
    _fields_ = [("near", C.c_double), ("far", C.c_double), ("flags", C.c_int32), ("pad", C.c_int32)]


class MwPlanTrace(C.Structure):
    _fields_ = [("agent_pos", C.c_void_p), ("agent_dir", C.c_void_p), ("carrying", C.c_void_p), ("ent_pos", C.c_void_p), ("ent_slot", C.c_int32)]


# the fields of a rollout trace (mw_plan_trace): name -> (dtype, per-env shape); ent_pos is ONE slot's position
TRACE_FIELDS = {
    "agent_pos": (np.float64, (3,)),
    "agent_dir": (np.float64, ()),
    "carrying": (np.int32, ()),
    "ent_pos": (np.float64, (3,)),
}


# name -> (dtype, per-env shape as a function of max_ents)
STATE_FIELDS = {
    "agent_pos": (np.float64, lambda E: (3,)),
    "agent_dir": (np.float64, lambda E: ()),
    "cam": (np.float64, lambda E: (4,)),
    "light": (np.float64, lambda E: (12,)),
    "carrying": (np.int32, lambda E: ()),
    "step_count": (np.int32, lambda E: ()),
    "num_picked_up": (np.int32, lambda E: ()),
    "ent_kind": (np.int32, lambda E: (E,)),
    "ent_mesh": (np.int32, lambda E: (E,)),
    "ent_static": (np.int32, lambda E: (E,)),
    "ent_pos": (np.float64, lambda E: (E, 3)),
    "ent_dir": (np.float64, lambda E: (E,)),
    "ent_geom": (np.float64, lambda E: (E, 9)),
    "extent": (np.float64, lambda E: (4,)),
}


class EngineError(RuntimeError):
    pass


def torch_dtype(dt):
    """the torch dtype of a field table's numpy type (STATE_FIELDS, TRACE_FIELDS)"""
    import torch
    return getattr(torch, np.dtype(dt).name)


def _sig(*argtypes, ret=C.c_int):
    return list(argtypes), ret


# The functions of include/mwengine.h: name -> (argtypes, restype), applied by load_library().  Handles and buffers are void pointers
# (the binding passes raw addresses), structs and host out-values are typed (tests/test_abi_mirror_cpu.py compares the table with the
# header: the names, each parameter's class, the return type).
vp, i32, i64, P = C.c_void_p, C.c_int32, C.c_int64, C.POINTER
SIGNATURES = {
    "mw_create": _sig(P(MwConfig), P(vp)),
    "mw_destroy": _sig(vp, ret=None),
    "mw_last_error": _sig(vp, ret=C.c_char_p),
    "mw_upload_texture": _sig(vp, i32, vp, i32, i32),
    "mw_upload_mesh": _sig(vp, i32, vp, vp, vp, vp, i32, i32),
    "mw_set_geometry": _sig(vp, i32, vp, i32, vp, i32),
    "mw_get_geometry": _sig(vp, i32, vp, P(i32), vp, P(i32)),
    "mw_set_state": _sig(vp, i32, i32, P(MwStateView)),
    "mw_get_state": _sig(vp, i32, i32, P(MwStateView)),
    "mw_get_state_device": _sig(vp, i32, i32, P(MwStateView), vp),
    "mw_set_state_where": _sig(vp, vp, P(MwStateView), vp),
    "mw_set_step_params": _sig(vp, vp),
    "mw_set_gen_program": _sig(vp, P(MwGenProgram), vp, vp, vp, vp, i32, vp, i32),
    "mw_reset": _sig(vp, vp, vp, vp),
    "mw_reset_where": _sig(vp, vp, vp, vp),
    "mw_set_reset_seeds": _sig(vp, vp),
    "mw_step": _sig(vp, vp, vp, vp, vp, vp, vp, vp),
    "mw_step_repeat": _sig(vp, vp, i32, vp, vp, vp, vp, vp, vp, vp),
    "mw_step_plan": _sig(vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp),
    "mw_step_plan_trace": _sig(vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, P(MwPlanTrace), vp),
    "mw_render": _sig(vp, vp, vp, vp),
    "mw_render_top": _sig(vp, vp, vp, i32, vp),
    "mw_render_view": _sig(vp, i32, i32, i32, i32, i32, vp, vp, vp),
    "mw_visible_ents": _sig(vp, i32, i32, vp, vp),
    "mw_set_obs_layout": _sig(vp, i32),
    "mw_set_final_obs": _sig(vp, vp, vp),
    "mw_set_frame_stack": _sig(vp, i32, i32, vp, vp),
    "mw_stack_refresh": _sig(vp, vp, vp),
    "mw_stack_window": _sig(vp, P(i32), P(i64)),
    "mw_snapshot_bytes": _sig(vp, i32, ret=i64),
    "mw_snapshot_save": _sig(vp, vp, i32, vp, i32, vp),
    "mw_snapshot_load": _sig(vp, vp, vp, i32, vp, i32, i32, vp),
    "mw_snapshot_frames_bytes": _sig(vp, i32, i32, ret=i64),
    "mw_snapshot_save_frames": _sig(vp, vp, i32, vp, vp, vp, i32, i32, vp),
    "mw_snapshot_load_frames": _sig(vp, vp, vp, i32, vp, i32, i32, i32, vp, vp, vp),
    "mw_snapshot_save_at": _sig(vp, vp, vp, i32, vp, i32, vp),
    "mw_snapshot_save_frames_at": _sig(vp, vp, vp, i32, vp, vp, vp, i32, i32, vp),
    "mw_snapshot_load_where": _sig(vp, vp, vp, vp, i32, i32, vp),
    "mw_snapshot_load_frames_where": _sig(vp, vp, vp, vp, i32, i32, i32, vp, vp, vp),
    "mw_nav_build": _sig(vp, P(MwNavParams), vp, vp, vp, vp),
    "mw_nav_build_grid": _sig(vp, P(MwNavParams), vp, vp, vp, vp, vp, vp, vp),
    "mw_nav_query": _sig(vp, P(MwNavParams), vp, vp, vp, vp, vp, vp, vp),
    "mw_debug_set_nav_passes": _sig(vp, vp),
    "mw_ray_cast": _sig(vp, P(MwRayParams), vp, vp, vp, vp, vp, vp, vp, vp),
    "mw_debug_set_ray_form": _sig(vp, C.c_int),
    "mw_grid_regions": _sig(vp, P(MwNavParams), i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp),
    "mw_seen_update": _sig(vp, P(MwNavParams), P(C.c_double), i32, vp, vp, vp, vp, vp, vp),
    "mw_grid_sight": _sig(vp, P(MwNavParams), P(C.c_double), i32, vp, vp, vp, vp, vp, vp, vp, vp),
    "mw_ego_map": _sig(vp, P(C.c_double), i32, i32, i32, vp, vp, vp, P(MwNavParams), vp, i32, C.c_uint32, vp, vp),
    "mw_depth_project": _sig(vp, P(C.c_double), vp, vp, i32, i32, vp, P(MwNavParams), i32, vp, vp, vp, vp, vp),
    "mw_label_frame": _sig(vp, vp, vp, vp, vp, vp, vp, vp, vp),        # (params: an MwLabelParams by reference)
    "mw_label_project": _sig(vp, P(C.c_double), vp, vp, i32, vp, i32, i32, vp, P(MwNavParams), vp, vp, i32, vp, vp, vp),
    "mw_debug_set_launch_shape": _sig(vp, C.c_int, C.c_int, C.c_int, C.c_int),
    "mw_pcg64_draws": _sig(C.c_uint64, i32, vp, vp),
    "mw_selftest_rcp": _sig(vp, vp, vp),
    "mw_selftest_div": _sig(vp, vp),
    "mw_selftest_sort": _sig(vp, vp, i32, vp),
    "mw_selftest_q": _sig(vp, vp),
    "mw_selftest_sincosf": _sig(vp, C.c_uint64, vp),
    "mw_check": _sig(vp, vp),
    "mw_kernel_time_ms": _sig(vp, i32, P(C.c_double), P(C.c_double), P(i64)),
    "mw_raster_path": _sig(vp),
    "mw_get_info": _sig(vp, vp, vp, i32, vp),
    "mw_get_final_info": _sig(vp, vp, vp, vp),
    "mw_get_reset_pending": _sig(vp, vp, vp),
    "mw_set_frame_reuse": _sig(vp, i32),
    "mw_get_frame_clean": _sig(vp, vp, vp),
    "mw_set_frame_cache": _sig(vp, i32),
    "mw_get_frame_source": _sig(vp, vp, vp),
    "mw_get_frame_plan": _sig(vp, vp, i64, vp, vp),
    "mw_get_geom_built": _sig(vp, vp, vp),
    "mw_get_list_lengths": _sig(vp, i32, i32, vp, vp),
    "mw_debug_set_mesh_frame_seq": _sig(vp, C.c_uint32),
    "mw_debug_get_slow_heads": _sig(vp, vp, vp),
}
EXPORTS = list(SIGNATURES)      # what a built library must export (__graft_entry__.build)

_said = set()


def build_library(force: bool = False) -> str:
    """Compile libmwengine.so for gfx950 with hipcc (in-tree); returns its path.  With MW_ENGINE_LIB set nothing is built: that file
    is what load_library() opens (a variant build made elsewhere; the in-tree sources say nothing about its age), said once."""
    if LIB_PATH != PRODUCT_PATH:
        if LIB_PATH not in _said:
            _said.add(LIB_PATH)
            print(f"miniworld_amd: MW_ENGINE_LIB is set: loading {LIB_PATH} as it is, not building {PRODUCT_PATH}", file=sys.stderr)
        return LIB_PATH
    srcs = [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith((".hip", ".h"))]
    srcs.append(os.path.join(_CSRC, "..", "..", "include", "mwengine.h"))
    stale = (not os.path.exists(LIB_PATH)) or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs)
    if force or stale:
        r = subprocess.run([os.path.join(_CSRC, "build.sh")], capture_output=True, text=True)
        if r.returncode != 0:
            raise EngineError("building libmwengine.so failed:\n" + r.stdout + r.stderr)
    return LIB_PATH


_lib = None


def load_library():
    """dlopen libmwengine.so and declare the C ABI.  Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    # torch first: its wheel bundles its own HIP runtime (libamdhip64); loading it before our
    # library makes both share ONE runtime instance (same soname), so device pointers and
    # streams can be exchanged.  The other order yields two runtimes in one process.
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise EngineError(
            f"{LIB_PATH} not found: the HIP engine is not built (run `python -c 'import __graft_entry__ as g; "
            "g.build()'` or miniworld_amd/csrc/build.sh).  There is no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    for name, (argtypes, restype) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.argtypes, fn.restype = argtypes, restype
    _lib = L
    return L


def frame_reuse_allowed() -> bool:
    """MW_FRAME_REUSE=0 forces frame reuse off, whatever a caller asks for: the A/B switch of an unchanged benchmark run."""
    return os.environ.get("MW_FRAME_REUSE", "1").strip() != "0"


MAX_FRAME_CACHE = 8     # MW_FC_MAX_SLOTS


def frame_cache_allowed() -> bool:
    """MW_FRAME_CACHE=0 forces the frame cache off, whatever a caller asks for: the A/B switch of an unchanged benchmark run."""
    return os.environ.get("MW_FRAME_CACHE", "1").strip() != "0"


def stack_slots(depth: int, push: int):
    """The ring rule of mw_set_frame_stack, once for host code and tests: push number `push` (0, 1, ...) of a stack of `depth`
    frames writes the frame to the slots `write_slots` of the env's 2 * depth - 1, and the ordered window after it is the `depth`
    consecutive slots from `window_first` on.  Returns (write_slots, window_first)."""
    p = push % depth
    return ((p + depth - 1,) if p == 0 else (p + depth - 1, p - 1)), p


def _stream_ptr(device=None):
    """torch's current stream ON THE ENGINE'S DEVICE (not on torch's current device)."""
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _ptr(t):
    """The device pointer of a tensor for the C ABI; None stays null."""
    return None if t is None else C.c_void_p(t.data_ptr())


class Engine:
    """One mw_engine: N environments resident on one GPU."""

    def __init__(self, cfg: MwConfig):
        self._init_host(cfg)
        self._open()

    def _init_host(self, cfg):
        """Every attribute the class reads that needs no device (a test without one replaces _open() alone)."""
        cfg.abi_version = ABI_VERSION
        self.cfg = cfg
        self.N = cfg.num_envs
        self.E = max(cfg.max_ents, 1)
        self.W, self.H = cfg.obs_width, cfg.obs_height
        self._set_layout(OBS_HWC_U8)
        self.frame_reuse = False
        self.frame_cache = 0
        self.lib = self.h = self.device = None

    def _open(self):
        """Where the engine lives: the library, the torch device and the mw_engine handle."""
        import torch
        if not torch.cuda.is_available():
            raise EngineError("no ROCm device visible: the mwengine HIP path cannot run (no CPU fallback exists)")
        self.lib = load_library()
        self.device = torch.device("cuda", self.cfg.device_id)
        h = C.c_void_p()
        rc = self.lib.mw_create(C.byref(self.cfg), C.byref(h))
        if rc != 0:
            raise EngineError(f"mw_create failed ({rc}): {self.lib.mw_last_error(None).decode()}")
        self.h = h

    def _check(self, rc, what):
        if rc != 0:
            raise EngineError(f"{what} failed ({rc}): {self.lib.mw_last_error(self.h).decode()}")

    def close(self):
        if getattr(self, "h", None):
            self.lib.mw_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- assets / world -------------------------------------------------------------
    def upload_texture(self, tex_id: int, rgb_bottom_up: np.ndarray):
        a = np.ascontiguousarray(rgb_bottom_up, np.uint8)
        assert a.ndim == 3 and a.shape[2] == 3
        self._check(self.lib.mw_upload_texture(self.h, tex_id, a.ctypes.data, a.shape[1], a.shape[0]), "mw_upload_texture")

    def upload_mesh(self, mesh_id: int, verts, norms, texcs, colors, tex_id: int = -1):
        """Per-face-vertex arrays [ntris][3][k] as built by miniworld_amd.objmesh.ObjMesh."""
        arrs = [np.ascontiguousarray(a, np.float32) for a in (verts, norms, texcs, colors)]
        n = arrs[0].shape[0]
        assert arrs[0].shape == (n, 3, 3) and arrs[1].shape == (n, 3, 3) and arrs[3].shape == (n, 3, 3)
        self._check(self.lib.mw_upload_mesh(self.h, mesh_id, arrs[0].ctypes.data, arrs[1].ctypes.data,
                                            arrs[2].ctypes.data, arrs[3].ctypes.data, n, tex_id), "mw_upload_mesh")

    def set_geometry(self, env: int, polys: np.ndarray, segs: np.ndarray):
        p = np.ascontiguousarray(polys, POLY_DTYPE)
        s = np.ascontiguousarray(segs, np.float64).reshape(-1, 4)
        self._check(self.lib.mw_set_geometry(self.h, env, p.ctypes.data, len(p), s.ctypes.data, len(s)), "mw_set_geometry")

    def get_geometry(self, env: int):
        polys = np.zeros(self.cfg.max_polys, POLY_DTYPE)
        segs = np.zeros((self.cfg.max_segs, 2, 2), np.float64)
        npoly, nseg = C.c_int32(), C.c_int32()
        self._check(self.lib.mw_get_geometry(self.h, env, polys.ctypes.data, C.byref(npoly), segs.ctypes.data,
                                             C.byref(nseg)), "mw_get_geometry")
        return polys[:npoly.value], segs[:nseg.value]

    def _view(self, arrays: dict, count: int, alloc: bool):
        view, keep = MwStateView(), {}
        for name, (dt, shp) in STATE_FIELDS.items():
            if alloc:
                arr = np.zeros((count,) + shp(self.E), dt)
            elif name in arrays and arrays[name] is not None:
                arr = np.ascontiguousarray(arrays[name], dt).reshape((count,) + shp(self.E))
            else:
                continue
            keep[name] = arr
            setattr(view, name, arr.ctypes.data)
        return view, keep

    def set_state(self, arrays: dict, first: int = 0, count: int | None = None):
        count = self.N - first if count is None else count
        view, keep = self._view(arrays, count, alloc=False)
        self._check(self.lib.mw_set_state(self.h, first, count, C.byref(view)), "mw_set_state")

    def get_state(self, first: int = 0, count: int | None = None) -> dict:
        count = self.N - first if count is None else count
        view, keep = self._view({}, count, alloc=True)
        self._check(self.lib.mw_get_state(self.h, first, count, C.byref(view)), "mw_get_state")
        return keep

    def _state_tensor(self, t, name, rows):
        """A field of a device-side state view: a contiguous tensor [rows, *field shape] of the field's dtype (float64 / int32) on the
        engine's device.  Checked, never converted: the kernels read raw pointers (_dev_tensor)."""
        if name not in STATE_FIELDS:
            raise EngineError(f"{name!r} is no state field; have {sorted(STATE_FIELDS)}")
        dt, shp = STATE_FIELDS[name]
        return self._shaped_tensor(t, name, torch_dtype(dt), (rows,) + shp(self.E))

    def _shaped_tensor(self, t, name, dtype, shape, more_rows=False):
        """A tensor whose shape matters beside its size: `shape` exactly (more_rows: shape[0] rows or more), then _dev_tensor's check."""
        import torch
        if not torch.is_tensor(t) or t.dim() != len(shape) or tuple(t.shape[1:]) != shape[1:] or (t.shape[0] < shape[0] if more_rows else t.shape[0] != shape[0]):
            raise EngineError(f"{name}: need a {dtype} tensor of shape {shape}{' or more rows' if more_rows else ''} on {self.device}, got "
                              f"{tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
        return self._dev_tensor(t, name, dtype, t.numel())

    def _device_view(self, tensors: dict, rows: int):
        view = MwStateView()
        for name, t in tensors.items():
            if t is None and name in STATE_FIELDS:      # (as for set_state: leave / do not fetch)
                continue
            setattr(view, name, self._state_tensor(t, name, rows).data_ptr())
        if not any(getattr(view, name) for name in STATE_FIELDS):
            raise EngineError("state view: no field named (every entry is None)")
        return view

    def get_state_device(self, out: dict | None = None, first: int = 0, count: int | None = None) -> dict:
        """get_state() on the device (mw_get_state_device): one kernel on the current stream, no synchronisation, no host value.
        `out` maps field names (those of get_state()) to device tensors [count, *field shape] of the field's dtype (float64 /
        int32), which are filled and returned; only the fields named are fetched.  None: every field, into new tensors.  The rows
        are bit for bit what get_state(first, count) would return at this point of the stream.  A tensor of another dtype,
        device, shape or stride pattern is refused before the library is called."""
        import torch
        count = self.N - first if count is None else count
        if first < 0 or count < 0 or first + count > self.N:
            raise EngineError(f"get_state_device: envs {first} .. {first + count - 1} of {self.N}")
        if out is None:
            out = {name: torch.zeros((count,) + shp(self.E), dtype=torch_dtype(dt), device=self.device)
                   for name, (dt, shp) in STATE_FIELDS.items()}
        if not out:
            raise EngineError("get_state_device: no field named")
        view = self._device_view(out, count)
        self._check(self.lib.mw_get_state_device(self.h, int(first), int(count), C.byref(view), _stream_ptr(self.device)), "mw_get_state_device")
        return out

    def set_state_where(self, mask, arrays: dict):
        """set_state() under a device mask (mw_set_state_where): for every env i with mask[i] != 0, row i of each tensor in `arrays`
        (field name -> device tensor [N, *field shape], float64 / int32) is written into the engine's state; rows under a zero mask
        byte are not read.  mask is a uint8[N] device tensor.  One kernel on the current stream, no synchronisation; the envs
        written lose their pending next-step reset, their frame-clean byte and their cached frames, every other env keeps its
        own.  Draw next (render), or step.  Nothing is converted: a wrong tensor is refused before the library is called."""
        mask = self._mask_tensor(mask)
        if not arrays:
            raise EngineError("set_state_where: no field named")
        view = self._device_view(arrays, self.N)
        self._check(self.lib.mw_set_state_where(self.h, _ptr(mask), C.byref(view), _stream_ptr(self.device)), "mw_set_state_where")

    # -- navigation fields ---------------------------------------------------------------
    def _nav_tensors(self, params: MwNavParams, field, target):
        import torch
        self._dev_tensor(field, "field", torch.uint16, self.N * params.gx * params.gz)
        self._dev_tensor(target, "target", torch.float64, self.N * 3)

    def nav_build(self, params: MwNavParams, field, mask=None, target=None):
        """mw_nav_build: rows of `field` (uint16[N, gz, gx], device) for the envs under `mask` (uint8[N], device; None = all) := the
        shortest-path cost to `target` (float64[N, 3], device; None = entity slot params.target_slot).  One kernel on the current
        stream, no synchronisation, nothing of the engine changes.  A wrong tensor is refused before the library is called."""
        self._nav_tensors(params, field, target)
        mask = self._mask_tensor(mask, optional=True)
        self._check(self.lib.mw_nav_build(self.h, C.byref(params), _ptr(mask), _ptr(target), _ptr(field), _stream_ptr(self.device)), "mw_nav_build")

    def nav_build_grid(self, params: MwNavParams, field, blocked, sources=None, target=None, extra=None, mask=None):
        """mw_nav_build_grid: rows of `field` (uint16[N, gz, gx], device) for the envs under `mask` := the shortest-path cost over the
        caller's own grids, each uint8[N, gz, gx] on the device: `blocked` (!= 0 a raw obstacle cell, inflated by params.margin metres),
        `sources` (!= 0 a source cell) and / or `target` (float64[N, 3] with params.reach), `extra` (a cost per cell; None = zeros).
        One kernel on the current stream, no synchronisation, nothing of the engine changes.  A wrong tensor is refused before the
        library is called."""
        import torch
        self._nav_tensors(params, field, target)
        cells = self.N * params.gx * params.gz
        for name, t in (("blocked", blocked), ("sources", sources), ("extra", extra)):
            self._dev_tensor(t, name, torch.uint8, cells)
        if blocked is None:
            raise EngineError("blocked: None")
        mask = self._mask_tensor(mask, optional=True)
        self._check(self.lib.mw_nav_build_grid(self.h, C.byref(params), _ptr(mask), _ptr(blocked), _ptr(sources), _ptr(target), _ptr(extra), _ptr(field),
                                               _stream_ptr(self.device)), "mw_nav_build_grid")

    def nav_query(self, params: MwNavParams, field, target=None, pos=None, cost=None, next=None, waypoint=None):
        """mw_nav_query: for the agents (pos None) or the rows of `pos` (float64[N, 3], device): cost int32[N], next int32[N] and
        waypoint float64[N, 2], whichever are given.  `target` as for the nav_build that made the field."""
        import torch
        self._nav_tensors(params, field, target)
        self._dev_tensor(pos, "pos", torch.float64, self.N * 3)
        self._dev_tensor(cost, "cost", torch.int32, self.N)
        self._dev_tensor(next, "next", torch.int32, self.N)
        self._dev_tensor(waypoint, "waypoint", torch.float64, self.N * 2)
        self._check(self.lib.mw_nav_query(self.h, C.byref(params), _ptr(target), _ptr(field), _ptr(pos), _ptr(cost), _ptr(next), _ptr(waypoint),
                                          _stream_ptr(self.device)), "mw_nav_query")

    def debug_set_nav_passes(self, passes):
        """Measurements: int32[N] on the device that every later nav_build or nav_build_grid fills with its relaxation's round count per env; None stops."""
        import torch
        self._dev_tensor(passes, "passes", torch.int32, self.N)
        self._nav_passes = passes       # (kept alive while the engine holds its pointer)
        self._check(self.lib.mw_debug_set_nav_passes(self.h, _ptr(passes)), "mw_debug_set_nav_passes")

    # -- ray casts -----------------------------------------------------------------------
    def ray_cast(self, params: MwRayParams, t, hit=None, dir_out=None, mask=None, origin=None, direction=None, offsets=None):
        """mw_ray_cast: R = params.rays rays per env under `mask` (uint8[N], device; None = all) from `origin` (float64[N, R, 3],
        device; None = the agents) along `direction` (float64[N, R, 2]) or the fan `offsets` (float64[R], radians from each agent's
        heading) into t (float64[N, R]), hit (int32[N, R]) and dir_out (float64[N, R, 2]), the last two optional.  One kernel on the
        current stream, no synchronisation, nothing of the engine changes.  A wrong tensor is refused before the library is called."""
        import torch
        n = self.N * int(params.rays)
        if t is None:
            raise EngineError("t: None")
        self._dev_tensor(t, "t", torch.float64, n)
        self._dev_tensor(hit, "hit", torch.int32, n)
        self._dev_tensor(dir_out, "dir_out", torch.float64, n * 2)
        self._dev_tensor(origin, "origin", torch.float64, n * 3)
        self._dev_tensor(direction, "direction", torch.float64, n * 2)
        self._dev_tensor(offsets, "offsets", torch.float64, int(params.rays))
        mask = self._mask_tensor(mask, optional=True)
        self._check(self.lib.mw_ray_cast(self.h, C.byref(params), _ptr(mask), _ptr(origin), _ptr(direction), _ptr(offsets), _ptr(t), _ptr(hit), _ptr(dir_out),
                                         _stream_ptr(self.device)), "mw_ray_cast")

    def debug_set_ray_form(self, form: int):
        """Measurements: 1 casts every ray count with a ray per lane, 2 with an obstacle per lane, 0 by the ray count again."""
        self._check(self.lib.mw_debug_set_ray_form(self.h, int(form)), "mw_debug_set_ray_form")

    # -- explored-area maps --------------------------------------------------------------
    def seen_update(self, params: MwNavParams, max_range: float, cos_half: float, flags: int, seen, count, new=None, mask=None, clear=None):
        """mw_seen_update: for the envs under `mask` (uint8[N], device; None = all) the cells of `seen` (uint8[N, gz, gx], device) each
        agent sees within `max_range` metres and the cone of cos(fov / 2) = `cos_half` (-1: all round) are set to 1, behind a zeroing
        of the rows under `clear` (uint8[N], device; None = none); new (int32[N], optional) gets the cells that went 0 -> 1, count
        (int32[N]) carries their sum.  One kernel on the current stream, no synchronisation, nothing of the engine changes.  A wrong
        tensor is refused before the library is called."""
        import torch
        if seen is None or count is None:
            raise EngineError(f"{'seen' if seen is None else 'count'}: None")
        self._shaped_tensor(seen, "seen", torch.uint8, (self.N, int(params.gz), int(params.gx)))
        self._dev_tensor(count, "count", torch.int32, self.N)
        self._dev_tensor(new, "new", torch.int32, self.N)
        self._dev_tensor(clear, "clear", torch.uint8, self.N)
        mask = self._mask_tensor(mask, optional=True)
        sight = (C.c_double * 2)(float(max_range), float(cos_half))
        self._check(self.lib.mw_seen_update(self.h, C.byref(params), sight, int(flags), _ptr(mask), _ptr(clear), _ptr(seen), _ptr(count), _ptr(new),
                                            _stream_ptr(self.device)), "mw_seen_update")

    # -- grid sight ----------------------------------------------------------------------
    def grid_sight(self, params: MwNavParams, max_range: float, cos_half: float, views: int, opaque, gain, weight=None, cells=None, dirs=None, seen=None,
                   mask=None):
        """mw_grid_sight: for the envs under `mask` (uint8[N], device; None = all) and each of `views` viewpoint cells — `cells`
        (int32[N, views], flat j * gx + i, device) with headings `dirs` (float64[N, views]; None: all round), or None: the agent's own
        cell and heading, views = 1 — gain (int32[N, views]) := the sum of `weight` (uint8[N, gz, gx]; None: the count) over the cells
        seen over `opaque` (uint8[N, gz, gx]) within `max_range` metres and the cone of cos(fov / 2) = `cos_half`; every seen cell of
        `seen` (uint8[N, gz, gx], optional) is set to 1.  One kernel on the current stream, no synchronisation, nothing of the engine
        changes.  A wrong tensor is refused before the library is called."""
        import torch
        if opaque is None or gain is None:
            raise EngineError(f"{'opaque' if opaque is None else 'gain'}: None")
        shape, views = (self.N, int(params.gz), int(params.gx)), int(views)
        self._shaped_tensor(opaque, "opaque", torch.uint8, shape)
        if weight is not None:
            self._shaped_tensor(weight, "weight", torch.uint8, shape)
        if seen is not None:
            self._shaped_tensor(seen, "seen", torch.uint8, shape)
        self._dev_tensor(gain, "gain", torch.int32, self.N * views)
        self._dev_tensor(cells, "cells", torch.int32, self.N * views)
        self._dev_tensor(dirs, "dirs", torch.float64, self.N * views)
        mask = self._mask_tensor(mask, optional=True)
        sight = (C.c_double * 2)(float(max_range), float(cos_half))
        self._check(self.lib.mw_grid_sight(self.h, C.byref(params), sight, views, _ptr(mask), _ptr(opaque), _ptr(weight), _ptr(cells), _ptr(dirs), _ptr(gain),
                                           _ptr(seen), _stream_ptr(self.device)), "mw_grid_sight")

    # -- grid regions --------------------------------------------------------------------
    def grid_regions(self, params: MwNavParams, connectivity: int, min_cells: int, max_regions: int, member, count, size, cell, sum=None, label=None,
                     mask=None):
        """mw_grid_regions: for the envs under `mask` (uint8[N], device; None = all) the connected regions (`connectivity` 4 or 8) of
        the bytes != 0 of `member` (uint8[N, gz, gx]): count (int32[N]) := the regions of at least `min_cells` cells, and for the first
        K = `max_regions` of them in the order of their lowest cells size (int32[N, K]), cell (int32[N, K]: the representative, flat
        j * gx + i, -1 for none), sum (int32[N, K, 2]: rows, columns; optional) and label (int16[N, gz, gx]: 0, k + 1 or -1; optional).
        One kernel on the current stream, no synchronisation, nothing of the engine changes.  A wrong tensor is refused before the
        library is called."""
        import torch
        for name, t in (("member", member), ("count", count), ("size", size), ("cell", cell)):
            if t is None:
                raise EngineError(f"{name}: None")
        shape, K = (self.N, int(params.gz), int(params.gx)), int(max_regions)
        self._shaped_tensor(member, "member", torch.uint8, shape)
        if label is not None:
            self._shaped_tensor(label, "label", torch.int16, shape)
        self._dev_tensor(count, "count", torch.int32, self.N)
        self._dev_tensor(size, "size", torch.int32, self.N * K)
        self._dev_tensor(cell, "cell", torch.int32, self.N * K)
        self._dev_tensor(sum, "sum", torch.int32, self.N * K * 2)
        mask = self._mask_tensor(mask, optional=True)
        self._check(self.lib.mw_grid_regions(self.h, C.byref(params), int(connectivity), int(min_cells), K, _ptr(mask), _ptr(member), _ptr(count), _ptr(size),
                                             _ptr(cell), _ptr(sum), _ptr(label), _stream_ptr(self.device)), "mw_grid_regions")

    # -- egocentric map windows ----------------------------------------------------------
    def ego_map(self, size: int, cell: float, back: float, wall_radius: float, entity_pad: float, max_range: float, cos_half: float, planes: int,
                flags: int, out=None, mask=None, pos=None, src_params: MwNavParams | None = None, src=None, fill: int = 0, sample=None):
        """mw_ego_map: for the envs under `mask` (uint8[N], device; None = all) the `size` x `size` window of points `cell` metres apart
        around each agent — or row i of `pos` (float64[N, 3], device) —, turned with its heading (EGO_NORTH in `flags`: not turned), `back`
        cells behind the centre: the planes named by the bits of `planes` (EGO_WALL, EGO_ENTITY, EGO_VISIBLE) into `out` (uint8[N, P, size,
        size], device; None iff planes == 0) and, with `src` (uint8 or uint16 [N, gz, gx] on the grid `src_params`), the source's element
        under every point, `fill` outside the grid, into `sample` ([N, size, size] of src's dtype).  One kernel on the current stream, no
        synchronisation, nothing of the engine changes.  A wrong tensor is refused before the library is called."""
        import torch
        size, planes = int(size), int(planes)
        count = bin(planes & (EGO_WALL | EGO_ENTITY | EGO_VISIBLE)).count("1")
        if (out is None) != (count == 0):
            raise EngineError("out: None" if out is None else "out: a tensor without planes to write")
        if out is not None:
            self._shaped_tensor(out, "out", torch.uint8, (self.N, count, size, size))
        self._dev_tensor(pos, "pos", torch.float64, self.N * 3)
        mask = self._mask_tensor(mask, optional=True)
        src_bytes = 0
        if src is not None:
            if src_params is None or sample is None:
                raise EngineError(f"{'src_params' if src_params is None else 'sample'}: None")
            if not torch.is_tensor(src) or src.dtype not in (torch.uint8, torch.uint16):
                raise EngineError(f"src: need a uint8 or uint16 tensor, got {src.dtype if torch.is_tensor(src) else type(src).__name__}")
            self._shaped_tensor(src, "src", src.dtype, (self.N, int(src_params.gz), int(src_params.gx)))
            self._shaped_tensor(sample, "sample", src.dtype, (self.N, size, size))
            src_bytes = src.element_size()
        elif sample is not None:
            raise EngineError("sample: a tensor without a source")
        window = (C.c_double * 6)(float(cell), float(back), float(wall_radius), float(entity_pad), float(max_range), float(cos_half))
        self._check(self.lib.mw_ego_map(self.h, window, size, planes, int(flags), _ptr(mask), _ptr(pos), _ptr(out),
                                        None if src is None else C.byref(src_params), _ptr(src), src_bytes, int(fill) & 0xFFFFFFFF, _ptr(sample),
                                        _stream_ptr(self.device)), "mw_ego_map")

    # -- depth projection ----------------------------------------------------------------
    def depth_project(self, depth, min_range: float, max_range: float, floor_tol: float, top: float, mask=None, size: int = 0, cell: float = 0.0,
                      back: float = 0.0, flags: int = 0, planes=None, params: MwNavParams | None = None, min_points: int = 1, map=None, count=None,
                      new=None, clear=None):
        """mw_depth_project: for the envs under `mask` (uint8[N], device; None = all) every pixel of `depth` (float32[N, H, W] or
        [N, H, W, 1], device) with min_range <= depth <= max_range is unprojected with the env's camera and the pose the device holds,
        classed as floor (|up| <= floor_tol) or obstacle (floor_tol < up <= top) and counted.  Window target (`planes`, uint8[N, 2, size,
        size]: the counts per cell of mw_ego_map's window of `size`, `cell`, `back`, EGO_NORTH in `flags`, clamped to 255) or map target
        (`params` with `map`, uint8[N, 2, gz, gx], `count` and optionally `new`, int32[N, 2]: a byte becomes 1 once the call's count reaches
        `min_points`, behind a zeroing of the rows under `clear`, uint8[N]).  One kernel on the current stream, no synchronisation, nothing
        of the engine changes.  A wrong tensor is refused before the library is called."""
        import torch
        H, W = self.H, self.W
        if not torch.is_tensor(depth) or tuple(depth.shape) not in ((self.N, H, W), (self.N, H, W, 1)):
            raise EngineError(f"depth: need a float32 tensor [{self.N}, {H}, {W}] or [{self.N}, {H}, {W}, 1], got "
                              f"{tuple(depth.shape) if torch.is_tensor(depth) else type(depth).__name__}")
        self._dev_tensor(depth, "depth", torch.float32, self.N * H * W)
        mask = self._mask_tensor(mask, optional=True)
        if (planes is None) == (params is None):
            raise EngineError("depth_project: exactly one target, planes (a window) or params with map (a map)")
        if params is None:
            self._shaped_tensor(planes, "planes", torch.uint8, (self.N, 2, int(size), int(size)))
            if map is not None or count is not None or new is not None or clear is not None:
                raise EngineError("depth_project: map, count, new and clear belong to the map target")
        else:
            if map is None or count is None:
                raise EngineError(f"{'map' if map is None else 'count'}: None")
            self._shaped_tensor(map, "map", torch.uint8, (self.N, 2, int(params.gz), int(params.gx)))
            self._shaped_tensor(count, "count", torch.int32, (self.N, 2))
            if new is not None:
                self._shaped_tensor(new, "new", torch.int32, (self.N, 2))
            self._dev_tensor(clear, "clear", torch.uint8, self.N)
        host = (C.c_double * 6)(float(min_range), float(max_range), float(floor_tol), float(top), float(cell), float(back))
        self._check(self.lib.mw_depth_project(self.h, host, _ptr(depth), _ptr(mask), int(size), int(flags), _ptr(planes),
                                              None if params is None else C.byref(params), int(min_points), _ptr(clear), _ptr(map), _ptr(count), _ptr(new),
                                              _stream_ptr(self.device)), "mw_depth_project")

    # -- label frames --------------------------------------------------------------------
    def label_frame(self, params: MwLabelParams, cls, code=None, depth=None, ent_pixels=None, ent_box=None, mask=None):
        """mw_label_frame: for the envs under `mask` (uint8[N], device; None = all) what every pixel of the env's observation shows — the
        first thing the ray through the pixel's depth sample meets among the static polygons, the Box slots and the mesh slots (their
        triangles, or with LABEL_MESH_BOUNDS in params.flags their cylinders) within params.near .. params.far of eye depth: `cls`
        (uint8[N, H, W], LABEL_*), `code` (int32[N, H, W]: a polygon's index, RAY_ENT + slot, -1), `depth` (float32[N, H, W]: the eye
        depth, far for nothing), `ent_pixels` (int32[N, E]) and `ent_box` (int32[N, E, 4]: u0, v0, u1, v1); every output but `cls` may be
        None.  One kernel on the current stream, no synchronisation, nothing of the engine changes.  A wrong tensor is refused before
        the library is called."""
        import torch
        if cls is None:
            raise EngineError("cls: None")
        mask = self._mask_tensor(mask, optional=True)
        for t, name, dtype, shape in ((cls, "cls", torch.uint8, (self.N, self.H, self.W)), (code, "code", torch.int32, (self.N, self.H, self.W)),
                                      (depth, "depth", torch.float32, (self.N, self.H, self.W)), (ent_pixels, "ent_pixels", torch.int32, (self.N, self.E)),
                                      (ent_box, "ent_box", torch.int32, (self.N, self.E, 4))):
            if t is not None:
                self._shaped_tensor(t, name, dtype, shape)
        self._check(self.lib.mw_label_frame(self.h, C.byref(params), _ptr(mask), _ptr(cls), _ptr(code), _ptr(depth), _ptr(ent_pixels), _ptr(ent_box),
                                            _stream_ptr(self.device)), "mw_label_frame")

    # -- object maps ---------------------------------------------------------------------
    def label_project(self, depth, code, base: int, min_range: float, max_range: float, floor_tol: float, top: float, mask=None, size: int = 0,
                      cell: float = 0.0, back: float = 0.0, flags: int = 0, plane=None, params: MwNavParams | None = None, map=None, clear=None, ids: int = 0,
                      cells=None, pos=None):
        """mw_label_project: for the envs under `mask` (uint8[N], device; None = all) every pixel of `depth` (float32[N, H, W] or
        [N, H, W, 1], device) that depth_project() would count carries the id `code - base` of `code` (int32[N, H, W], device) — 0 .. 254,
        anything else "no object" — into its cell, which keeps the lowest id.  Window target (`plane`, uint8[N, size, size]: 1 + id, 0 for
        none, of mw_ego_map's window of `size`, `cell`, `back`, EGO_NORTH in `flags`) or map target (`params` with `map`, uint8[N, gz, gx]:
        a cell the frame saw is rewritten, the others keep their byte, behind a rewrite of every byte of the rows under `clear`, uint8[N];
        with `ids` > 0 `cells`, int32[N, ids], and `pos`, float64[N, ids, 3], at least one of them: how many cells of the map hold each id
        and their centroid, NaN for none).  One kernel on the current stream, no synchronisation, nothing of the engine changes.  A wrong
        tensor is refused before the library is called."""
        import torch
        H, W = self.H, self.W
        if not torch.is_tensor(depth) or tuple(depth.shape) not in ((self.N, H, W), (self.N, H, W, 1)):
            raise EngineError(f"depth: need a float32 tensor [{self.N}, {H}, {W}] or [{self.N}, {H}, {W}, 1], got "
                              f"{tuple(depth.shape) if torch.is_tensor(depth) else type(depth).__name__}")
        self._dev_tensor(depth, "depth", torch.float32, self.N * H * W)
        self._shaped_tensor(code, "code", torch.int32, (self.N, H, W))
        mask = self._mask_tensor(mask, optional=True)
        if (plane is None) == (params is None):
            raise EngineError("label_project: exactly one target, plane (a window) or params with map (a map)")
        if params is None:
            self._shaped_tensor(plane, "plane", torch.uint8, (self.N, int(size), int(size)))
            if map is not None or clear is not None or cells is not None or pos is not None:
                raise EngineError("label_project: map, clear, cells and pos belong to the map target")
        else:
            if map is None:
                raise EngineError("map: None")
            self._shaped_tensor(map, "map", torch.uint8, (self.N, int(params.gz), int(params.gx)))
            if cells is not None:
                self._shaped_tensor(cells, "cells", torch.int32, (self.N, int(ids)))
            if pos is not None:
                self._shaped_tensor(pos, "pos", torch.float64, (self.N, int(ids), 3))
            self._dev_tensor(clear, "clear", torch.uint8, self.N)
        host = (C.c_double * 6)(float(min_range), float(max_range), float(floor_tol), float(top), float(cell), float(back))
        self._check(self.lib.mw_label_project(self.h, host, _ptr(depth), _ptr(code), int(base), _ptr(mask), int(size), int(flags), _ptr(plane),
                                              None if params is None else C.byref(params), _ptr(clear), _ptr(map), int(ids), _ptr(cells), _ptr(pos),
                                              _stream_ptr(self.device)), "mw_label_project")

    def debug_set_launch_shape(self, waves_per_env: int = 0, mesh_tile_waves: int = 0, ent_blocks: int = 0, slow_waves: int = 0):
        """Tests and measurements: wavefronts per env of the tile kernels (a divisor of the frame's tile count) and the persistent
        workers of the mesh tiles (>= 8), the mesh entity kernel (>= 8) and the mesh slow path (>= 1); 0 keeps a value.  Every
        frame is the same bits under every shape."""
        self._check(self.lib.mw_debug_set_launch_shape(self.h, int(waves_per_env), int(mesh_tile_waves), int(ent_blocks), int(slow_waves)),
                    "mw_debug_set_launch_shape")

    def set_gen_program(self, prog: MwGenProgram, polys: np.ndarray, poly_room, poly_surf, poly_m, segs: np.ndarray):
        """Installs the placement program of an MW_GEN_PROGRAM engine (include/mwengine.h: mw_set_gen_program)."""
        p = np.ascontiguousarray(polys, POLY_DTYPE)
        room = np.ascontiguousarray(poly_room, np.int32)
        surf = np.ascontiguousarray(poly_surf, np.int32)
        m = np.ascontiguousarray(poly_m, np.float64).reshape(len(p), 4, 2)
        sg = np.ascontiguousarray(segs, np.float64).reshape(-1, 4)
        self._check(self.lib.mw_set_gen_program(self.h, C.byref(prog), p.ctypes.data, room.ctypes.data, surf.ctypes.data,
                                                m.ctypes.data, len(p), sg.ctypes.data, len(sg)), "mw_set_gen_program")

    def set_step_params(self, params: np.ndarray | None):
        p = None if params is None else np.ascontiguousarray(params, np.float64).reshape(self.N, 3)
        self._check(self.lib.mw_set_step_params(self.h, None if p is None else p.ctypes.data), "mw_set_step_params")

    def reset(self, mask: np.ndarray | None = None, seeds: np.ndarray | None = None):
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        s = None if seeds is None else np.ascontiguousarray(seeds, np.uint64)
        self._check(self.lib.mw_reset(self.h, None if m is None else m.ctypes.data,
                                      None if s is None else s.ctypes.data, _stream_ptr(self.device)), "mw_reset")

    def _seed_tensor(self, seeds, name):
        """Seeds the device reads: a contiguous int64[N] tensor on the engine's device, whose bits the engine takes as uint64
        (torch's own integer type; a non-negative int64 is the same number).  Nothing is converted or read here."""
        import torch
        if seeds is None:
            raise EngineError(f"{name}: None")
        return self._dev_tensor(seeds, name, torch.int64, self.N)

    def reset_where(self, mask, seeds):
        """reset(mask, seeds) with both arrays on the device (mw_reset_where): for every env i with mask[i] != 0 the episode of
        env.reset(seed=seeds[i]) starts — stream re-seeded and world generated on the device, no host synchronisation, no copy of the
        stream array.  mask uint8[N], seeds int64[N] (bits as uint64; not read under a zero mask byte), device tensors, nothing is
        converted.  The other envs, their streams and their cached frames are untouched.  Asynchronous on the current stream; draw
        next (render)."""
        mask, seeds = self._mask_tensor(mask), self._seed_tensor(seeds, "seeds")
        self._check(self.lib.mw_reset_where(self.h, _ptr(mask), _ptr(seeds), _stream_ptr(self.device)), "mw_reset_where")

    def set_reset_seeds(self, next_seed=None):
        """Seeded same-step auto-reset (mw_set_reset_seeds): with `next_seed`, an int64[N] device tensor (bits as uint64), an env whose
        episode ends in a step starts the episode of env.reset(seed=next_seed[i]) in that step.  The engine reads next_seed[i] only
        for an env that finishes, when it finishes: write the tensor between steps, on the stream the steps run on.  None turns it
        off.  The engine keeps a reference to the tensor while it is in use."""
        if next_seed is not None:
            self._seed_tensor(next_seed, "next_seed")
        self._check(self.lib.mw_set_reset_seeds(self.h, _ptr(next_seed)), "mw_set_reset_seeds")
        self._reset_seeds = next_seed

    # -- hot path ---------------------------------------------------------------------
    def _dev_tensor(self, t, name, dtype, numel, at_least=False):
        """The kernels read raw pointers: a tensor of another dtype / device / stride pattern would be read as garbage
        (an int64 action tensor as int32 pairs, a CPU tensor as a fault).  Outputs must already be right; see step().
        at_least: a buffer that may be larger than what is written (record buffers, the rows of step_reward)."""
        if t is None:
            return None
        if t.device != self.device or t.dtype != dtype or not t.is_contiguous() or (t.numel() < numel if at_least else t.numel() != numel):
            raise EngineError(f"{name}: need a contiguous {dtype} tensor of {'at least ' if at_least else ''}{numel} elements on {self.device}, got "
                              f"{t.dtype} {tuple(t.shape)} on {t.device}{'' if t.is_contiguous() else ' (non-contiguous)'}")
        return t

    def _set_layout(self, layout):
        """obs_layout, and with it obs_spec: the (dtype, elements per frame) of an observation in that layout — the one place"""
        import torch
        self.obs_layout = int(layout)
        self.obs_spec = (torch.float64, self.H * self.W) if self.obs_layout == OBS_GREY_F64 else (torch.uint8, self.H * self.W * 3)

    def _obs_tensor(self, obs, name="obs"):
        """a buffer of N frames in the current layout (obs_buffer()'s dtype and size), or None"""
        dtype, per_frame = self.obs_spec
        return self._dev_tensor(obs, name, dtype, self.N * per_frame)

    def _depth_tensor(self, depth, name="depth"):
        """float32 [N, H, W] depth, or None"""
        import torch
        return self._dev_tensor(depth, name, torch.float32, self.N * self.H * self.W)

    def _step_tensors(self, actions, obs, depth, reward, term, trunc):
        """The checks step() and step_repeat() share; returns the int32 actions."""
        import torch
        if actions.device != self.device or actions.dtype != torch.int32 or not actions.is_contiguous():
            actions = actions.to(device=self.device, dtype=torch.int32).contiguous()
        if actions.numel() != self.N:
            raise EngineError(f"actions: {actions.numel()} elements for {self.N} envs")
        dtype, per_frame = self.obs_spec        # (_obs_tensor and _depth_tensor, written out: this is every step's path)
        self._dev_tensor(obs, "obs", dtype, self.N * per_frame)
        self._dev_tensor(depth, "depth", torch.float32, self.N * self.H * self.W)
        self._dev_tensor(reward, "reward", torch.float32, self.N)
        self._dev_tensor(term, "terminated", torch.uint8, self.N)
        self._dev_tensor(trunc, "truncated", torch.uint8, self.N)
        return actions

    def step(self, actions, obs, depth=None, reward=None, term=None, trunc=None):
        """All arguments are torch tensors on this engine's device (depth may be None).  `actions` is converted to a
        contiguous int32 tensor on the device if it is not one already (torch.randint / argmax / Categorical.sample
        give int64; a column of a [N, T] tensor is strided); the output tensors are checked, never converted."""
        actions = self._step_tensors(actions, obs, depth, reward, term, trunc)
        self._check(self.lib.mw_step(self.h, _ptr(actions), _ptr(obs), _ptr(depth), _ptr(reward), _ptr(term),
                                     _ptr(trunc), _stream_ptr(self.device)), "mw_step")

    def step_repeat(self, actions, repeat, obs, depth=None, reward=None, term=None, trunc=None, nsteps=None):
        """Action repeat (include/mwengine.h: mw_step_repeat): every env takes up to `repeat` steps with its action, stops at
        the one that ends its episode, and one frame is drawn at the end.  Tensors as for step(); `nsteps`, int32[N] or None,
        receives the sub-steps each env executed.  `repeat` outside 1 .. MAX_REPEAT raises before the library is called."""
        import torch
        if not isinstance(repeat, (int, np.integer)) or not 1 <= repeat <= MAX_REPEAT:
            raise EngineError(f"repeat: need an integer in 1 .. {MAX_REPEAT}, got {repeat!r}")
        actions = self._step_tensors(actions, obs, depth, reward, term, trunc)
        self._dev_tensor(nsteps, "nsteps", torch.int32, self.N)
        self._check(self.lib.mw_step_repeat(self.h, _ptr(actions), int(repeat), _ptr(obs), _ptr(depth), _ptr(reward), _ptr(term),
                                            _ptr(trunc), _ptr(nsteps), _stream_ptr(self.device)), "mw_step_repeat")

    def step_plan(self, plans, obs, depth=None, reward=None, step_reward=None, term=None, trunc=None, nsteps=None):
        """Open-loop rollout (include/mwengine.h: mw_step_plan): `plans` is an integer tensor [T, N], env i takes plans[0, i],
        plans[1, i], ... until its episode ends, in one step-kernel launch.  It is converted to contiguous int32 on the device if
        needed; the outputs are checked as for step_repeat(), `step_reward` (float32, at least T * N elements: rows 0 .. T - 1 of a
        [*, N] buffer) receives every sub-step's own reward.  obs=None is the frameless call: nothing is drawn, `depth` must be None.
        A wrong shape or T outside 1 .. MAX_PLAN raises before the library is called."""
        self._step_plan(plans, obs, depth, reward, step_reward, term, trunc, nsteps, None)

    def step_plan_trace(self, plans, obs, depth=None, reward=None, step_reward=None, term=None, trunc=None, nsteps=None, *, trace: dict,
                        ent_slot: int = 0):
        """step_plan() with a trace (include/mwengine.h: mw_step_plan_trace): `trace` maps names of TRACE_FIELDS to device tensors
        [R, N, *field shape] with R >= T rows — "agent_pos" float64[R, N, 3], "agent_dir" float64[R, N], "carrying" int32[R, N],
        "ent_pos" float64[R, N, 3] (the position of slot `ent_slot`) — whose row k receives every env's state after its sub-step k,
        rows an env did not execute repeating its last one; rows T .. R - 1 are not written.  Everything else is step_plan()'s.
        Checked like a state view's tensors (dtype, device, contiguity), never converted: an unknown name, a wrong tensor, no field
        at all, ent_pos with a slot outside 0 .. max_ents - 1 or on a TASK_COLLECT engine raise before the library is called."""
        if not trace or all(t is None for t in trace.values()):
            raise EngineError("step_plan_trace: no trace field named")
        view = MwPlanTrace()
        T = int(plans.shape[0]) if plans.dim() == 2 else 0
        for name, t in trace.items():
            if name not in TRACE_FIELDS:
                raise EngineError(f"{name!r} is no trace field; have {sorted(TRACE_FIELDS)}")
            if t is None:
                continue
            dt, shp = TRACE_FIELDS[name]
            setattr(view, name, self._shaped_tensor(t, "trace " + name, torch_dtype(dt), (T, self.N) + shp, more_rows=True).data_ptr())
        if view.ent_pos:
            if isinstance(ent_slot, bool) or not isinstance(ent_slot, (int, np.integer)) or not 0 <= ent_slot < self.cfg.max_ents:
                raise EngineError(f"ent_slot: need an integer in 0 .. {self.cfg.max_ents - 1}, got {ent_slot!r}")
            if self.cfg.task == TASK_COLLECT:
                raise EngineError("trace ent_pos on a TASK_COLLECT engine: a kit's respawn belongs to the frame's tail")
            view.ent_slot = int(ent_slot)
        self._step_plan(plans, obs, depth, reward, step_reward, term, trunc, nsteps, view)

    def _step_plan(self, plans, obs, depth, reward, step_reward, term, trunc, nsteps, trace):
        """step_plan() and step_plan_trace(): the checks, then the one library call (trace: the filled MwPlanTrace or None)."""
        import torch
        if plans.dim() != 2 or plans.shape[1] != self.N or not 1 <= plans.shape[0] <= MAX_PLAN:
            raise EngineError(f"plans: need an integer tensor [T, {self.N}] with T in 1 .. {MAX_PLAN}, got {tuple(plans.shape)}")
        horizon = int(plans.shape[0])
        if obs is None and depth is not None:
            raise EngineError("step_plan: depth without obs (a frameless call draws nothing)")
        if plans.device != self.device or plans.dtype != torch.int32 or not plans.is_contiguous():
            plans = plans.to(device=self.device, dtype=torch.int32).contiguous()
        self._step_tensors(plans[0], obs, depth, reward, term, trunc)       # (the output checks; row 0 stands in for step()'s actions)
        self._dev_tensor(nsteps, "nsteps", torch.int32, self.N)
        self._dev_tensor(step_reward, "step_reward", torch.float32, horizon * self.N, at_least=True)
        fn, tail = ("mw_step_plan", ()) if trace is None else ("mw_step_plan_trace", (C.byref(trace),))
        self._check(getattr(self.lib, fn)(self.h, _ptr(plans), horizon, _ptr(obs), _ptr(depth), _ptr(reward), _ptr(step_reward), _ptr(term),
                                          _ptr(trunc), _ptr(nsteps), *tail, _stream_ptr(self.device)), fn)

    def set_final_obs(self, obs=None, depth=None):
        """Same-step auto-reset: every later step writes the terminal frame (and depth) of each env whose episode ended in it into
        that env's row of `obs` (`depth`); the other rows are left alone.  Device tensors shaped like the step's obs / depth
        (obs_buffer()); obs=None turns it off.  The engine keeps references to them while they are in use."""
        if obs is not None:
            self._obs_tensor(obs, "final obs")
            self._depth_tensor(depth, "final depth")
        self._check(self.lib.mw_set_final_obs(self.h, _ptr(obs), _ptr(depth if obs is not None else None)), "mw_set_final_obs")
        self._final_bufs = (obs, depth) if obs is not None else None

    def set_frame_stack(self, depth: int, pad: int = STACK_PAD_RESET, ring=None, final_stack=None):
        """Frame stacking on the device (include/mwengine.h: mw_set_frame_stack): every later step() / step_repeat() pushes its
        frame into `ring`, a device tensor of [N, 2 * depth - 1, *frame] elements in the obs dtype, and — on an engine with final
        buffers — completes the rows of `final_stack` ([N, depth, *frame]) of the envs whose episode ended.  depth = 0 or
        ring=None turns it off.  The engine keeps references to the tensors while they are in use."""
        if depth and ring is not None:
            dtype, per_frame = self.obs_spec
            self._dev_tensor(ring, "stack ring", dtype, self.N * (2 * depth - 1) * per_frame)
            self._dev_tensor(final_stack, "final stack", dtype, self.N * depth * per_frame)
        else:
            depth, ring, final_stack = 0, None, None
        self._check(self.lib.mw_set_frame_stack(self.h, int(depth), int(pad), _ptr(ring), _ptr(final_stack)), "mw_set_frame_stack")
        self._stack_bufs = (ring, final_stack) if depth else None

    def stack_refresh(self, obs):
        """The reset path of the frame stack: after reset(mask) and render(obs), rebuilds the stacks of the envs that were reset (or
        never pushed) from their rows of `obs`; the others and the ring position stay (mw_stack_refresh)."""
        self._check(self.lib.mw_stack_refresh(self.h, _ptr(obs), _stream_ptr(self.device)), "mw_stack_refresh")

    def stack_window(self):
        """(first_slot, pushes): every env's ordered stack is ring[:, first_slot : first_slot + depth]; host values, no sync."""
        first, pushes = C.c_int32(), C.c_int64()
        self._check(self.lib.mw_stack_window(self.h, C.byref(first), C.byref(pushes)), "mw_stack_window")
        return first.value, pushes.value

    # -- snapshots ---------------------------------------------------------------------
    def snapshot_bytes(self, capacity: int) -> int:
        """Bytes of a device buffer that holds `capacity` records of this engine (include/mwengine.h: mw_snapshot_bytes)."""
        n = int(self.lib.mw_snapshot_bytes(self.h, int(capacity)))
        if n < 0:
            raise EngineError(f"mw_snapshot_bytes failed ({n}): capacity {capacity!r}")
        return n

    def _index_tensor(self, t, name, count=None):
        """An index array of a snapshot call: None, or made a contiguous int32 tensor on the engine's device."""
        import torch
        if t is None:
            return None
        t = torch.as_tensor(t)
        if t.device != self.device or t.dtype != torch.int32 or not t.is_contiguous():
            t = t.to(device=self.device, dtype=torch.int32).contiguous()
        if t.dim() != 1 or (count is not None and t.numel() != count):
            raise EngineError(f"{name}: need a 1-D index tensor" + (f" of {count} elements" if count is not None else "") + f", got shape {tuple(t.shape)}")
        return t

    def _items(self, envs, records, count, default):
        """The index tensors and the item count of a list call: envs / records None or made int32 device tensors (_index_tensor), count
        the length of whichever is given, else `default`; every array given must be that long."""
        envs, records = self._index_tensor(envs, "envs"), self._index_tensor(records, "records")
        if count is None:
            count = envs.numel() if envs is not None else records.numel() if records is not None else default
        for t, name in ((envs, "envs"), (records, "records")):
            if t is not None and t.numel() != count:
                raise EngineError(f"{name}: {t.numel()} indices for {count} items")
        return envs, records, int(count)

    def _where_items(self, mask, records, instead):
        """The mask and the record indices of a _where call: uint8[N] as given, int32[N] made a device tensor."""
        mask, records = self._mask_tensor(mask), self._index_tensor(records, "records", self.N)
        if records is None:
            raise EngineError(f"records: None (record i for env i: {instead})")
        return mask, records

    def _records_call(self, fn, buf, capacity, frames, *args):
        """What the snapshot calls share behind their indices: the record buffer's check — with `frames` = (obs, depth, flags), a
        frame record call, the frame rows' too —, then the library call fn(handle, *args, stream)."""
        import torch
        if frames is None:
            self._dev_tensor(buf, f"snapshot buffer for {capacity} records", torch.uint8, self.snapshot_bytes(capacity), at_least=True)
        else:
            obs, depth, flags = frames
            self._dev_tensor(buf, f"frame record buffer for {capacity} records (flags {flags})", torch.uint8,
                             self.snapshot_frames_bytes(capacity, flags), at_least=True)
            self._frame_rows(obs, depth, flags)
        self._check(getattr(self.lib, fn)(self.h, *args, _stream_ptr(self.device)), fn)

    def snapshot_save(self, buf, capacity: int, envs=None, count: int | None = None):
        """Record k of `buf` := the complete state of env envs[k] (envs=None: env k, for k < count, default all envs); `buf` is a
        uint8 device tensor of snapshot_bytes(capacity) bytes.  Asynchronous on the current stream, one kernel; returns the number
        of records written (mw_snapshot_save)."""
        envs, _, count = self._items(envs, None, count, self.N)
        self._records_call("mw_snapshot_save", buf, capacity, None, _ptr(envs), count, _ptr(buf), int(capacity))
        return count

    def snapshot_load(self, buf, n_recs: int, capacity: int, envs=None, records=None, count: int | None = None):
        """Env envs[k] := record records[k] of `buf`, whose first n_recs records are valid (envs=None: env k; records=None: record
        k).  The target envs must be distinct; records may repeat — a fork.  The observation buffers are stale afterwards: render(),
        then stack_refresh() with a frame stack (mw_snapshot_load).  Asynchronous on the current stream, one kernel."""
        envs, records, count = self._items(envs, records, count, min(int(n_recs), self.N))
        self._records_call("mw_snapshot_load", buf, capacity, None, _ptr(envs), _ptr(records), count, _ptr(buf), int(n_recs), int(capacity))

    def snapshot_frames_bytes(self, capacity: int, flags: int = 0) -> int:
        """Bytes of a device buffer that holds `capacity` frame records under `flags` (SNAPF_DEPTH | SNAPF_STACK;
        include/mwengine.h: mw_snapshot_frames_bytes)."""
        n = int(self.lib.mw_snapshot_frames_bytes(self.h, int(capacity), int(flags)))
        if n < 0:
            raise EngineError(f"mw_snapshot_frames_bytes failed ({n}): capacity {capacity!r}, flags {flags!r}")
        return n

    def _frame_rows(self, obs, depth, flags):
        """The kernels index `obs` / `depth` by env through raw pointers: they must be the step's buffers (obs_buffer()'s dtype and
        size in the current layout, float32 [N, H, W] depth), and SNAPF_DEPTH needs a depth tensor."""
        if obs is None:
            raise EngineError("frame records: obs is None")
        self._obs_tensor(obs)
        if (flags & SNAPF_DEPTH) and depth is None:
            raise EngineError("frame records: SNAPF_DEPTH without a depth tensor")
        self._depth_tensor(depth)

    def snapshot_save_frames(self, buf, capacity: int, obs, depth=None, flags: int = 0, envs=None, count: int | None = None):
        """Frame record k of `buf` := env envs[k]'s row of `obs`, with SNAPF_DEPTH its row of `depth`, with SNAPF_STACK its stacked
        frames and stack flag (envs=None: env k, for k < count, default all envs); `buf` is a uint8 device tensor of
        snapshot_frames_bytes(capacity, flags) bytes that overlaps none of them.  Asynchronous on the current stream, one kernel;
        returns the number of records written (mw_snapshot_save_frames)."""
        envs, _, count = self._items(envs, None, count, self.N)
        self._records_call("mw_snapshot_save_frames", buf, capacity, (obs, depth, flags),
                           _ptr(envs), count, _ptr(obs), _ptr(depth), _ptr(buf), int(capacity), int(flags))
        return count

    def snapshot_load_frames(self, buf, n_recs: int, capacity: int, obs, depth=None, flags: int = 0, envs=None, records=None,
                             count: int | None = None):
        """Env envs[k]'s rows of `obs` / `depth` (and with SNAPF_STACK its frame stack and stack flag) := frame record records[k] of
        `buf`, saved under the same `flags`.  Called behind snapshot_load() with the same indices it replaces render() and
        stack_refresh(): the frames are the ones the records' sources returned.  Asynchronous on the current stream, one kernel
        (mw_snapshot_load_frames)."""
        envs, records, count = self._items(envs, records, count, min(int(n_recs), self.N))
        self._records_call("mw_snapshot_load_frames", buf, capacity, (obs, depth, flags),
                           _ptr(envs), _ptr(records), count, _ptr(buf), int(n_recs), int(capacity), int(flags), _ptr(obs), _ptr(depth))

    def snapshot_save_at(self, buf, capacity: int, envs=None, records=None, count: int | None = None):
        """Record records[k] of `buf` := the complete state of env envs[k] (envs=None: env k; records=None: record k).  The records
        named must be distinct; every other record of `buf` keeps what it held, so a bank of more records than the engine has envs
        is filled in chunks and a running loop adds to it.  Asynchronous on the current stream, one kernel; returns the number of
        records written (mw_snapshot_save_at)."""
        envs, records, count = self._items(envs, records, count, self.N)
        self._records_call("mw_snapshot_save_at", buf, capacity, None, _ptr(envs), _ptr(records), count, _ptr(buf), int(capacity))
        return count

    def snapshot_save_frames_at(self, buf, capacity: int, obs, depth=None, flags: int = 0, envs=None, records=None, count: int | None = None):
        """Frame record records[k] of `buf` := env envs[k]'s frames, as snapshot_save_frames() takes them; the other records keep
        what they held (mw_snapshot_save_frames_at).  Asynchronous on the current stream, one kernel; returns the number written."""
        envs, records, count = self._items(envs, records, count, self.N)
        self._records_call("mw_snapshot_save_frames_at", buf, capacity, (obs, depth, flags),
                           _ptr(envs), _ptr(records), count, _ptr(obs), _ptr(depth), _ptr(buf), int(capacity), int(flags))
        return count

    def _mask_tensor(self, mask, optional=False):
        """The mask of a _where call: a contiguous uint8[N] tensor on the engine's device (nothing is converted: a conversion
        would be a kernel and an allocation in every step of the loop this call exists for); None only where it means every env."""
        import torch
        if mask is None and not optional:
            raise EngineError("mask: None")
        return self._dev_tensor(mask, "mask", torch.uint8, self.N)

    def snapshot_load_where(self, buf, n_recs: int, capacity: int, mask, records):
        """For every env i with mask[i] != 0: env i := record records[i] of `buf`, whose first n_recs records are valid.  mask uint8[N]
        and records int32[N] are device tensors; nothing is read on the host, so the call sits behind a step with no
        synchronisation.  records[i] is not read under a zero mask byte; N may exceed `capacity` (records repeat).  The other
        envs keep their cached frames (mw_snapshot_load_where).  Asynchronous on the current stream, one kernel."""
        mask, records = self._where_items(mask, records, "snapshot_load")
        self._records_call("mw_snapshot_load_where", buf, capacity, None, _ptr(mask), _ptr(records), _ptr(buf), int(n_recs), int(capacity))

    def snapshot_load_frames_where(self, buf, n_recs: int, capacity: int, mask, records, obs, depth=None, flags: int = 0):
        """For every env i with mask[i] != 0: env i's rows of `obs` / `depth` (and with SNAPF_STACK its frame stack and stack flag) :=
        frame record records[i] of `buf`; no byte of any other env's rows is touched.  Called behind snapshot_load_where() with the
        same mask and records (mw_snapshot_load_frames_where).  Asynchronous on the current stream, one kernel."""
        mask, records = self._where_items(mask, records, "snapshot_load_frames")
        self._records_call("mw_snapshot_load_frames_where", buf, capacity, (obs, depth, flags),
                           _ptr(mask), _ptr(records), _ptr(buf), int(n_recs), int(capacity), int(flags), _ptr(obs), _ptr(depth))

    def render(self, obs, depth=None):
        self._check(self.lib.mw_render(self.h, _ptr(obs), _ptr(depth), _stream_ptr(self.device)), "mw_render")

    def render_top(self, obs, depth=None, render_agent=True):
        self._check(self.lib.mw_render_top(self.h, _ptr(obs), _ptr(depth), int(render_agent), _stream_ptr(self.device)), "mw_render_top")

    def render_view(self, env: int, width: int, height: int, msaa: int = 16, top: bool = False,
                    render_agent: bool = False, want_depth: bool = False):
        """One env into a (height, width) buffer with 8 or 16 samples; returns torch tensors."""
        import torch
        out = torch.zeros((height, width, 3), dtype=torch.uint8, device=self.device)
        dep = torch.zeros((height, width, 1), dtype=torch.float32, device=self.device) if want_depth else None
        flags = (1 if top else 0) | (2 if render_agent else 0)
        self._check(self.lib.mw_render_view(self.h, env, flags, width, height, msaa, _ptr(out), _ptr(dep), _stream_ptr(self.device)),
                    "mw_render_view")
        return (out, dep) if want_depth else out

    def set_obs_layout(self, layout: int):
        """Layout of the obs buffer the raster kernel writes: OBS_HWC_U8 | OBS_CWH_U8 | OBS_GREY_F64."""
        self._check(self.lib.mw_set_obs_layout(self.h, int(layout)), "mw_set_obs_layout")
        self._set_layout(layout)

    def obs_buffer(self, count: int | None = None):
        """A device tensor of the right shape / dtype for the current obs layout."""
        import torch
        frame = {OBS_CWH_U8: (3, self.W, self.H), OBS_GREY_F64: (self.H, self.W, 1)}.get(self.obs_layout, (self.H, self.W, 3))
        return torch.zeros((self.N if count is None else count,) + frame, dtype=self.obs_spec[0], device=self.device)

    def visible_ents(self, first_env: int = 0, count: int | None = None):
        """get_visible_ents (miniworld.py:1238-1333): uint8[count, max_ents] on the device, 1 = visible."""
        import torch
        count = self.N - first_env if count is None else count
        vis = torch.zeros((count, self.E), dtype=torch.uint8, device=self.device)
        self._check(self.lib.mw_visible_ents(self.h, first_env, count, _ptr(vis), _stream_ptr(self.device)),
                    "mw_visible_ents")
        return vis

    def check(self):
        self._check(self.lib.mw_check(self.h, _stream_ptr(self.device)), "mw_check")

    def _info_tensors(self, health, pos):
        """what get_info and get_final_info ask of their outputs: int32[N] and float64[N, 3] device tensors, either may be None"""
        import torch
        self._dev_tensor(health, "health", torch.int32, self.N)
        self._dev_tensor(pos, "position", torch.float64, self.N * 3)

    def get_info(self, health=None, ent_pos=None, ent_slot=0):
        """Fills the caller's device tensors: health int32[N] (CollectHealth's info["health"]) and / or ent_pos float64[N, 3]
        (position of entity slot ent_slot: TMaze / YMaze info["goal_pos"])."""
        self._info_tensors(health, ent_pos)
        self._check(self.lib.mw_get_info(self.h, _ptr(health), _ptr(ent_pos), int(ent_slot), _stream_ptr(self.device)), "mw_get_info")

    def get_final_info(self, health=None, goal_pos=None):
        """The `info` values of each env's last FINISHED episode (kept by the step kernel before the same-step auto-reset): health
        int32[N] (CollectHealth) and / or goal_pos float64[N, 3] (TMaze / YMaze)."""
        self._info_tensors(health, goal_pos)
        self._check(self.lib.mw_get_final_info(self.h, _ptr(health), _ptr(goal_pos), _stream_ptr(self.device)), "mw_get_final_info")

    def _get_bytes(self, fn, out):
        """a uint8[N] getter of the library into `out`, made here when None"""
        import torch
        if out is None:
            out = torch.zeros(self.N, dtype=torch.uint8, device=self.device)
        self._dev_tensor(out, fn, torch.uint8, self.N)
        self._check(getattr(self.lib, fn)(self.h, _ptr(out), _stream_ptr(self.device)), fn)
        return out

    def get_reset_pending(self, out=None):
        """uint8[N] on the device: 1 = the env's last step ended its episode and, under AUTORESET_NEXT_STEP, its next step installs
        the next world instead of stepping (the action is ignored; reward 0, flags 0).  Written into `out` when given."""
        return self._get_bytes("mw_get_reset_pending", out)

    def set_frame_reuse(self, on: bool):
        """Lets step() leave the rows of envs whose frame did not change undrawn (include/mwengine.h: mw_set_frame_reuse).  With
        it on the caller promises to pass the same obs / depth tensors to consecutive steps and not to write to them in
        between.  MW_FRAME_REUSE=0 in the environment forces it off (the A/B switch); returns what is in effect."""
        on = bool(on) and frame_reuse_allowed()
        self._check(self.lib.mw_set_frame_reuse(self.h, int(on)), "mw_set_frame_reuse")
        self.frame_reuse = on
        return on

    def set_frame_cache(self, slots: int):
        """The engine keeps every env's last `slots` distinct drawn frames (0 .. MAX_FRAME_CACHE, 0 = off) and copies one instead
        of drawing when the env is back in the state it shows (include/mwengine.h: mw_set_frame_cache; num_envs x slots x H x W x 3
        bytes, and as many floats with depth).  MW_FRAME_CACHE=0 in the environment forces it off (the A/B switch); returns what is
        in effect."""
        slots = int(slots) if frame_cache_allowed() else 0
        self._check(self.lib.mw_set_frame_cache(self.h, slots), "mw_set_frame_cache")
        self.frame_cache = slots
        return slots

    def get_frame_source(self, out=None):
        """uint8[N] on the device: where each env's frame of the last plain step came from — 0 drawn, 1 left alone as clean (frame
        reuse), 2 + j copied from slot j of the frame cache.  Written into `out` when given."""
        return self._get_bytes("mw_get_frame_source", out)

    def get_frame_plan(self):
        """Test and diagnosis call (synchronises): the plan the last planned frame was drawn from (include/mwengine.h:
        mw_get_frame_plan), as a dict — `classes` (8 in an ordered plan, 0 in an unordered one), `class_counts` (the draw entries per
        cost class), `draw` (uint32, the draw entries env | victim slot << 24 in the order the quad kernel's workgroups take them:
        the highest class first), `copy` (the copy entries env | slot << 24), `lengths` (int32[N], every env's display-list length,
        the cost input: class = min(7, length // 4)) and `block`, the raw words."""
        N = self.N
        ordered = N <= 0xFFFF
        block = np.zeros(96 + N * (9 if ordered else 2), np.uint32)
        lengths = np.zeros(N, np.int32)
        self._check(self.lib.mw_get_frame_plan(self.h, block.ctypes.data, block.size, lengths.ctypes.data, _stream_ptr(self.device)), "mw_get_frame_plan")
        n_draw, n_copy, classes = int(block[0]), int(block[1]), int(block[2])
        packed = [int(block[32]) | int(block[33]) << 32, int(block[64]) | int(block[65]) << 32]
        counts = [(packed[c >> 2] >> (16 * (c & 3))) & 0xFFFF for c in range(8)] if classes else []
        if classes:
            draw = np.concatenate([block[96 + N * (1 + c):96 + N * (1 + c) + min(counts[c], N)] for c in reversed(range(8))])
        else:
            draw = block[96 + N:96 + N + min(n_draw, N)].copy()
        return {"n_draw": n_draw, "n_copy": n_copy, "classes": classes, "class_counts": counts, "draw": draw,
                "copy": block[96:96 + min(n_copy, N)].copy(), "lengths": lengths, "block": block}

    def get_geom_built(self):
        """Test and diagnosis call (synchronises): uint8[N], 1 where the geometry kernel of the last planned frame built the env's
        display list, 0 where it left the list, its length and the header of an earlier frame (include/mwengine.h: mw_get_geom_built)."""
        out = np.zeros(self.N, np.uint8)
        self._check(self.lib.mw_get_geom_built(self.h, out.ctypes.data, _stream_ptr(self.device)), "mw_get_geom_built")
        return out

    def get_frame_clean(self, out=None):
        """uint8[N] on the device: 1 = the env's frame after the last step is bit for bit the frame before it (a blocked move, a
        pickup that found nothing ...), whether or not reuse is on.  Written into `out` when given."""
        return self._get_bytes("mw_get_frame_clean", out)

    def list_lengths(self):
        """int32[N]: triangles in each env's display list of the last frame (after clipping and culling); of its last build for an
        env that a planned frame did not build (get_geom_built)."""
        out = np.zeros(self.N, np.int32)
        self._check(self.lib.mw_get_list_lengths(self.h, 0, self.N, out.ctypes.data, _stream_ptr(self.device)), "mw_get_list_lengths")
        return out

    def raster_path(self):
        """Which raster kernels drew the last frame: PATH_TILE / PATH_QUAD / PATH_QUAD_MESH / PATH_GENERIC (mwengine.h)."""
        return int(self.lib.mw_raster_path(self.h))

    def kernel_time_ms(self, reset=0):
        """(raster ms, setup ms, launches measured) since the last call; reset = k > 0: time one launch in k from now
        on (1 = every launch), 0: the default one in 8, < 0: switch timing off."""
        r, s, n = C.c_double(), C.c_double(), C.c_int64()
        self._check(self.lib.mw_kernel_time_ms(self.h, reset, C.byref(r), C.byref(s), C.byref(n)), "mw_kernel_time_ms")
        return r.value, s.value, n.value


# ------------------------------------------------------------------ DomainParams -> config

def default_ranges() -> dict:
    """The reference's DEFAULT_PARAMS table (params.py:115-130) as (default, min, max)."""
    return {
        "sky_color": ([0.25, 0.82, 1.0], [0.1, 0.1, 0.1], [1.0, 1.0, 1.0]),
        "light_pos": ([0, 2.5, 0], [-40, 2.5, -40], [40, 5, 40]),
        "light_color": ([0.7, 0.7, 0.7], [0.45, 0.45, 0.45], [0.8, 0.8, 0.8]),
        "light_ambient": ([0.45, 0.45, 0.45], [0.35, 0.35, 0.35], [0.55, 0.55, 0.55]),
        "obj_color_bias": ([0, 0, 0], [-0.2, -0.2, -0.2], [0.2, 0.2, 0.2]),
        "forward_step": (0.15, 0.12, 0.17),
        "forward_drift": (0.0, -0.05, 0.05),
        "turn_step": (15.0, 10.0, 20.0),
        "cam_pitch": (0.0, -5.0, 5.0),
        "cam_fov_y": (60.0, 55.0, 65.0),
        "cam_height": (1.5, 1.45, 1.55),
        "cam_fwd_disp": (0.0, -0.05, 0.10),
    }


def fill_ranges(cfg: MwConfig, ranges: dict | None = None):
    r = default_ranges() if ranges is None else ranges
    for name in ("forward_step", "forward_drift", "turn_step", "cam_pitch", "cam_fov_y", "cam_height", "cam_fwd_disp"):
        setattr(cfg, name, MwRange.of(*r[name]))
    for name in ("sky_color", "light_pos", "light_color", "light_ambient", "obj_color_bias"):
        d, lo, hi = r[name]
        arr = getattr(cfg, name)
        for k in range(3):
            arr[k] = MwRange.of(d[k], lo[k], hi[k])
    cfg.max_forward_step = float(r["forward_step"][2])
