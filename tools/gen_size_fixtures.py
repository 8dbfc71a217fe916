"""Generates tests/golden/sizes/*.npz: frames of the REFERENCE ITSELF at observation and window sizes that are not multiples
of the engine's 16 x 4 raster tile (FIXTURE TOOLING, build container only).

The sibling of tools/gen_gl_fixtures.py: the same unmodified reference on Mesa llvmpipe (tools/refshim_gl.py), the same
trajectories (tools/gen_golden.py's cases), but the env is built with obs_width / obs_height (and window_width /
window_height for render()) of the case's size.  Stored per frame k, as gen_gl_fixtures.py stores them:
  gl/<k>/scene/*, gl/<k>/rgb, z16, depth, top, vis, and for the frames listed in VIEW: gl/<k>/view_agent at the window size.
meta/frames, meta/env, meta/size (W, H), meta/window (W, H), meta/samples.  The fixtures live in their own directory:
tests/conftest.py and tests/test_oracle_vs_reference_gl.py pick up every tests/golden/*.npz at the top level.
While generating, every frame is compared with the oracle and the statistics are printed.

Usage:  python tools/gen_size_fixtures.py [--one-spp] [case ...]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_gl_fixtures as glf  # noqa: E402  (cases(), read_z16(), mesh_arrays(), the oracle and the GL shim)

pyoracle, refscene, refshim_gl = glf.pyoracle, glf.refscene, glf.refshim_gl
OUT = os.path.join(HERE, "..", "tests", "golden", "sizes")
SIZES = [(84, 84), (81, 61)]
CASES = ["hallway_s0", "pickup_dr_s1", "maze_s0"]
N_FRAMES = 2                                     # the first frames of the case's list
VIEW = {("hallway_s0", 84, 84): 7}               # one render() frame at WINDOW
WINDOW = (801, 601)
ONE_SPP = [("hallway_s0", 81, 61)]               # --one-spp: the reference's single-sampled fallback (gen_gl_fixtures.py)


def capture(env, out, k, stats, ns, W, H, view):
    sc = refscene.scene_from_ref_env(env)
    meshes = glf.mesh_arrays(env)
    ents = [e for e in env.entities if e is not env.agent]
    rgb = env.render_obs().copy()
    z16 = glf.read_z16(env, env.obs_fb)
    depth = env.render_depth().copy()
    top = env.render_top_view(env.obs_fb).copy()
    visible = env.get_visible_ents()
    vis = np.array([any(e is v for v in visible) for e in ents], bool)
    for key, val in sc.items():
        out[f"gl/{k}/scene/{key}"] = val
    out[f"gl/{k}/rgb"], out[f"gl/{k}/z16"], out[f"gl/{k}/depth"], out[f"gl/{k}/top"], out[f"gl/{k}/vis"] = rgb, z16, depth, top, vis
    r = pyoracle.render(sc, width=W, height=H, nsamples=ns, meshes=meshes)
    t = pyoracle.render(sc, width=W, height=H, nsamples=ns, meshes=meshes, view="top", render_agent=True)
    v = pyoracle.visible_ents(sc, width=W, height=H, nsamples=ns)
    stats["frames"] += 1
    stats["rgb_bad"] += int((r["rgb"] != rgb).any(axis=2).sum())
    stats["z_bad"] += int((r["z16"] != z16).sum())
    stats["depth_bad"] += int((r["depth"].view(np.uint32) != depth.view(np.uint32)).sum())
    stats["top_bad"] += int((t["rgb"] != top).any(axis=2).sum())
    stats["vis_bad"] += int((v != vis).sum())
    if view:
        env.render_mode = "rgb_array"
        env.view = "agent"
        img = env.render().copy()
        out[f"gl/{k}/view_agent"] = img
        rr = pyoracle.render(sc, width=WINDOW[0], height=WINDOW[1], nsamples=ns, meshes=meshes, view="agent")
        stats["view_bad"] += int((rr["rgb"] != img).any(axis=2).sum())


def run_case(case, W, H, ns, prefix):
    name, cls, kwargs, seed, n_actions, steps, frames = case
    frames = frames[:N_FRAMES]
    view_at = VIEW.get((name, W, H)) if ns > 1 else None
    env = refshim_gl.make_env(cls, obs_width=W, obs_height=H, window_width=WINDOW[0], window_height=WINDOW[1], **kwargs)
    env.reset(seed=seed)
    rng = np.random.default_rng(1000 + seed)            # the action stream of tools/gen_golden.py
    out = {}
    stats = dict(frames=0, rgb_bad=0, z_bad=0, depth_bad=0, top_bad=0, vis_bad=0, view_bad=0)
    done = []
    last = max(frames + ([view_at] if view_at is not None else []))
    for t in range(last + 1):
        if t in frames or t == view_at:
            capture(env, out, t, stats, ns, W, H, view=(t == view_at))
            done.append(t)
        if t == last:
            break
        if isinstance(n_actions, list):
            a = int(rng.choice(len(n_actions), p=n_actions))
        else:
            a = int(rng.integers(0, n_actions))
        _, _, term, trunc, _ = env.step(a)
        if term or trunc:
            break
    out["meta/frames"] = np.array(done, np.int32)
    out["meta/env"] = np.array(cls)
    out["meta/size"] = np.array([W, H], np.int32)
    out["meta/window"] = np.array(WINDOW, np.int32)
    out["meta/samples"] = np.array(ns, np.int32)
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, f"{prefix}{name}_{W}x{H}.npz"), **out)
    print(f"{prefix}{name} {W}x{H}: {stats}")


def main():
    args = sys.argv[1:]
    table = {c[0]: c for c in glf.cases()}
    if "--one-spp" in args:
        args.remove("--one-spp")
        os.environ["MW_REF_FORCE_1SPP"] = "1"
        for name, W, H in ONE_SPP:
            if not args or name in args:
                run_case(table[name], W, H, 1, "gl1_")
        return
    for name in CASES:
        if args and name not in args:
            continue
        for W, H in SIZES:
            run_case(table[name], W, H, 4, "gl_")


if __name__ == "__main__":
    main()
