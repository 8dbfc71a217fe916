"""Out-of-sample differential test: the CPU oracle against the REFERENCE ITSELF, on states no other fixture holds.

tests/golden/gl_*.npz pin the oracle on 101 states of tools/gen_golden.py's table; tests/golden/unseen/*.npz hold 50 more,
drawn as (family, seed, steps, domain_rand, view) triples from a seeded generator of their own (tools/ref_random_diff.py
--save: the reference, unmodified, on Mesa llvmpipe), and this test demands oracle == reference bit for bit on them: RGB, the
16-bit depth buffer and the float32 depth map.  Every registered family appears at least once.  Regenerating the fixtures
re-runs the reference and prints the same comparison; tools/debug/gl_vs_oracle.py is the hand-held version of the check.
"""
import os

import numpy as np

import helpers
import pyoracle
from conftest import GOLDEN

FAMILIES = 23       # the registered env families


def _load(name):
    d = np.load(os.path.join(GOLDEN, "unseen", name))
    meta = {f: d[f"meta/{f}"] for f in ("cls", "seed", "steps", "domain_rand", "top")}
    kd = {key[len("mesh_kd/"):]: d[key] for key in d.files if key.startswith("mesh_kd/")}
    cases = []
    for k in range(len(meta["cls"])):
        pre = f"case/{k}/"
        sc = {key[len(pre) + 6:]: d[key] for key in d.files if key.startswith(pre + "scene/")}
        fr = {key[len(pre):]: d[key] for key in d.files if key.startswith(pre) and not key.startswith(pre + "scene/")}
        c = {f: meta[f][k].item() for f in meta}
        cases.append((c, sc, fr))
    return d, kd, cases


def _diff(name, nsamples):
    """The oracle on every stored state: one result per case like tools/ref_random_diff.py's, plus the fixture's metadata."""
    d, kd, cases = _load(name)
    results = []
    for c, sc, fr in cases:
        meshes = helpers.golden_meshes(sc)
        for m in meshes:          # the material colour the reference gave each mesh (meshes.npz holds the geometry)
            meshes[m]["colors"] = np.broadcast_to(kd[m].astype(np.float32), meshes[m]["verts"].shape).copy()
        r = pyoracle.render(sc, nsamples=nsamples, meshes=meshes, view="top" if c["top"] else "agent", render_agent=c["top"])
        res = dict(c)
        res["rgb_bad"] = int(np.count_nonzero(fr["rgb"] != r["rgb"]))
        res["z_bad"] = int(np.count_nonzero(fr["z16"] != r["z16"]))
        res["depth_bad"] = 0 if c["top"] else int(np.count_nonzero(fr["depth"].view(np.uint32) != r["depth"].view(np.uint32)))
        res["mean"] = float(fr["rgb"].mean())
        results.append(res)
    bad = [r for r in results if r["rgb_bad"] or r["z_bad"] or r["depth_bad"]]
    return {"cases": len(results), "bad": bad, "families": sorted({r["cls"] for r in results}), "driver": str(d["meta/driver"]),
            "samples": int(d["meta/samples"]), "results": results}


def test_oracle_equals_the_reference_on_unseen_states():
    """46 triples (every one of the 23 families twice), 4 samples per pixel: llvmpipe's GL_MAX_SAMPLES, what the reference's
    FrameBuffer falls back to (opengl.py:229-231)."""
    j = _diff("ref_4spp_60601.npz", 4)
    assert "llvmpipe" in j["driver"] and j["samples"] == 4
    assert j["cases"] == 46 and len(j["families"]) == FAMILIES
    assert any(r["top"] for r in j["results"]) and any(r["domain_rand"] for r in j["results"]) and any(r["steps"] > 30 for r in j["results"])
    assert all(1.0 < r["mean"] < 254.0 for r in j["results"])            # real frames
    assert not j["bad"], f"oracle != reference on {[(b['cls'], b['seed'], b['steps'], b['domain_rand'], b['top'], b['rgb_bad'], b['z_bad'], b['depth_bad']) for b in j['bad']]}"


def test_oracle_equals_the_reference_single_sampled_fallback_on_unseen_states():
    """The other fallback (opengl.py:263-284): glTexImage2DMultisample fails, FrameBuffer renders single-sampled."""
    j = _diff("ref_1spp_60602.npz", 1)
    assert j["samples"] == 1 and j["cases"] == 4
    assert not j["bad"], f"oracle != reference (1 sample) on {[(b['cls'], b['seed'], b['steps'], b['rgb_bad'], b['z_bad']) for b in j['bad']]}"
