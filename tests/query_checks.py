"""What the tests of the world queries share (nav fields, ray casts, seen maps, ego windows, depth projection, label frames;
tests/test_*_cpu.py and tests/test_gpu_*.py of each): the sanitizer build of a tests/hostcheck program and the run of one on a file,
the host worlds and walks the files are made of, the checks of a query's interface, and the few lines every GPU module starts with.
A plain module: the restatements (*_reference.py) stay independent of it and of each other."""
import math
import os
import re
import subprocess

import numpy as np

import nav_reference as nav

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "miniworld_amd", "csrc")


# ---------------------------------------------------------------------------------------------------------------- the programs

def build(name, dir):
    """hostcheck/<name>.cpp under the address and undefined-behaviour sanitizers, as a program of its own in `dir`: the executable"""
    exe = str(dir / name)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", os.path.join(HERE, "hostcheck", name + ".cpp"), "-o", exe])
    return exe


def world_lines(w, carry=False, pose=False, extent=True):
    """the world block of a program's file (hostcheck/hostcheck.h): AGENT, with CARRY and POSE where asked, EXTENT unless not, SEGS, SLOTS"""
    lines = [f"{w['agent_radius']!r} {w['max_forward_step']!r}" + (f" {w['carry']}" if carry else "")]
    if pose:
        lines.append(" ".join(repr(float(v)) for v in w["agent"]))
    if extent:
        lines.append(" ".join(repr(float(v)) for v in w["extent"]))
    lines.append(str(len(w["segs"])))
    lines += [" ".join(repr(float(v)) for v in s) for s in w["segs"]]
    lines.append(str(len(w["kind"])))
    for s in range(len(w["kind"])):
        lines.append(f"{int(w['kind'][s])} " + " ".join(repr(float(v)) for v in w["pos"][s]) + f" {float(w['radius'][s])!r}")
    return lines


def run(program, path, lines, timeout=300, blank=False):
    """writes `lines` to `path`, runs the program on it and returns the rows of its answer — without the blank ones unless `blank`
    (a row of no elements is blank)"""
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([program, str(path)], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stdout[-300:], r.stderr[-2000:])
    rows = r.stdout.split("\n")[:-1]
    return rows if blank else [row for row in rows if row]


LAUNCH = ("grid", "threads", "lds", "fits")


def launch_of(program, *args, names=LAUNCH):
    """`program --policy args...`: the launch it prints, by name"""
    out = subprocess.run([program, "--policy"] + [str(a) for a in args], capture_output=True, text=True, check=True).stdout.split()
    return dict(zip(names, map(int, out)))


# ---------------------------------------------------------------------------------------------------------------- the worlds

_scenes = {}


def scene(cls_name, seed=0):
    """the scene of a host class after reset(seed), made once; callers copy before they change it"""
    if (cls_name, seed) not in _scenes:
        from miniworld_amd import envs
        from miniworld_amd.scene import scene_from_env
        env = getattr(envs, cls_name)(host_only=True)
        env.reset(seed=seed)
        _scenes[(cls_name, seed)] = scene_from_env(env)
    return _scenes[(cls_name, seed)]


def host_world(cls_name, seed):
    """(env, scene, world): a fresh host env after reset(seed), and the restatements' world of it with the agent's pose (x, z, dir)"""
    from miniworld_amd import envs
    from miniworld_amd.scene import scene_from_env
    env = getattr(envs, cls_name)(host_only=True)
    env.reset(seed=seed)
    sc = scene_from_env(env)
    w = nav.world_of_scene(sc)
    w["agent"] = pose_of(sc)
    return env, sc, w


def pose_of(sc):
    return (float(sc["agent_pos"][0]), float(sc["agent_pos"][2]), float(sc["agent_dir"]))


def pose_walk(extent, pose, rng, steps, turn, step, margin):
    """poses (x, z, dir) from `pose`: turns of `turn` degrees and forward moves of `step` metres, one draw of `rng` each, kept `margin`
    inside the extent"""
    x, z, d = pose
    out = [(x, z, d)]
    for _ in range(steps - 1):
        a = rng.integers(0, 3)
        if a == 0:
            d += math.radians(turn)
        elif a == 1:
            d -= math.radians(turn)
        else:
            x = min(max(x + step * math.cos(d), extent[0] + margin), extent[1] - margin)
            z = min(max(z - step * math.sin(d), extent[2] + margin), extent[3] - margin)
        out.append((x, z, d))
    return out


def walk(w, rng, steps):
    """poses (x, z, dir): from the agent's own, forward moves and turns of the env's sizes, kept inside the extent"""
    return pose_walk(w["extent"], w["agent"], rng, steps, 15, 0.45, 0.1)


def scene_walk(cls_name, steps, seed, rng_seed, turn):
    """poses (x, z, dir) from the scene's own first one: turns and short forward moves, kept well inside the extent"""
    sc = scene(cls_name, seed)
    return pose_walk([float(v) for v in sc["extent"]], pose_of(sc), np.random.default_rng(rng_seed), steps, turn, 0.15, 0.5)


# ---------------------------------------------------------------------------------------------------------------- the interface

def check_units_built(*units):
    make = open(os.path.join(CSRC, "Makefile")).read()
    for unit in units:
        assert re.search(r"^SRCS = (?:.*\\\n)*.*\b" + re.escape(unit), make, re.M), unit


def check_kernel(kernel, unit):
    """mw_kernels.h declares the kernel, once, and `unit` defines it, once"""
    decl = open(os.path.join(CSRC, "mw_kernels.h")).read()
    assert len(re.findall(r'extern "C" __global__ void ' + kernel + r"\(", decl)) == 1, kernel
    assert len(re.findall(r"__global__[^;{]*\b" + kernel + r"\(", open(os.path.join(CSRC, unit)).read())) == 1, kernel


def check_does_not_wait(unit):
    """the engine unit says why its call does not wait for the side-stream refills"""
    assert "does not wait for the Maze's" in " ".join(open(os.path.join(CSRC, unit)).read().replace("//", " ").split()), unit


def check_refuses_null_engine(name, *args):
    """the library exports `name`, and the call with a null engine and `args` returns -1"""
    from miniworld_amd import engine
    engine.build_library()
    lib = engine.load_library()
    assert hasattr(lib, name), name
    assert getattr(lib, name)(None, *args) == -1, name


# ---------------------------------------------------------------------------------------------------------------- on the GPU

def vec_env(env_id, n, **kw):
    """a reset MiniWorldVecEnv, seed 0 unless given"""
    from miniworld_amd.vec_env import MiniWorldVecEnv
    kw.setdefault("seed", 0)
    vec = MiniWorldVecEnv(env_id, n, **kw)
    vec.reset()
    return vec


def worlds(vec):
    """the restatements' world of every env, from the host route"""
    st = vec.engine.get_state()
    return [nav.world_of_engine(vec.engine, st, i) for i in range(vec.num_envs)]


def poses(vec):
    st = vec.state(("agent_pos", "agent_dir"))
    pos, d = st["agent_pos"].cpu().numpy(), st["agent_dir"].cpu().numpy()
    return [(pos[i, 0], pos[i, 2], d[i]) for i in range(vec.num_envs)]


def teleport(vec, xz, direction=None):
    """every agent to xz = (x[N], z[N]) — and to one heading — by a device-side state write"""
    import torch
    pos = vec.state(("agent_pos",))["agent_pos"].clone()
    pos[:, 0], pos[:, 2] = torch.as_tensor(xz[0], dtype=torch.float64, device="cuda"), torch.as_tensor(xz[1], dtype=torch.float64, device="cuda")
    fields = {"agent_pos": pos}
    if direction is not None:
        fields["agent_dir"] = torch.as_tensor(direction, dtype=torch.float64, device="cuda").expand(vec.num_envs).contiguous()
    vec.set_state_where(torch.ones(vec.num_envs, dtype=torch.uint8, device="cuda"), **fields)


def dev(a, dtype=None):
    """None, or `a` as a device tensor (of numpy's dtype unless one is given)"""
    import torch
    return None if a is None else torch.as_tensor(np.asarray(a), device="cuda", dtype=dtype)


def host(t):
    """a device tensor as numpy; uint16 through its bits"""
    import torch
    return t.view(torch.int16).cpu().numpy().view(np.uint16) if t.dtype == torch.uint16 else t.cpu().numpy()
