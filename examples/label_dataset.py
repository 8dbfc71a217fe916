#!/usr/bin/env python3
"""A detection / segmentation data set from a stepping batch, with no host value in the loop: PickupObjects under domain randomisation,
random actions, and per kept step the observation, the class plane of a label frame (`vec.label_frame()`, `vec.label_update()`: what
every pixel shows — floor, wall, Box, mesh object ..., cast on the device from the live world) and the per-slot boxes, copied into
device buffers.  Thresholding colours cannot do this here: the randomisation moves them.

    python examples/label_dataset.py --envs 256 --steps 200 --keep-every 4

Prints the share of pixels per class over the kept steps and the share of kept (env, step) pairs with an object — any Box or mesh slot —
in view, both computed on the device after the loop.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

CLASSES = ("nothing", "floor", "ceiling", "wall", "frame", "box", "mesh")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="MiniWorld-PickupObjects-v0")
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--keep-every", type=int, default=4)
    ap.add_argument("--meshes", choices=["exact", "bounds"], default="exact")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    n, kept = args.envs, (args.steps + args.keep_every - 1) // args.keep_every
    vec = MiniWorldVecEnv(args.env, n, seed=args.seed, domain_rand=True)
    dev = vec.engine.device
    vec.reset()
    f = vec.label_frame(meshes=args.meshes, code=False, stats=True)
    obs = torch.zeros((kept,) + tuple(vec.obs.shape), dtype=torch.uint8, device=dev)
    cls = torch.zeros((kept,) + tuple(f.cls.shape), dtype=torch.uint8, device=dev)
    boxes = torch.zeros((kept,) + tuple(f.ent_box.shape), dtype=torch.int32, device=dev)
    g = torch.Generator(device=dev).manual_seed(args.seed)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(args.steps):
        vec.step(torch.randint(0, 3, (n,), generator=g, device=dev, dtype=torch.int32))
        if t % args.keep_every == 0:
            vec.label_update(f)
            k = t // args.keep_every
            obs[k].copy_(vec.obs)
            cls[k].copy_(f.cls)
            boxes[k].copy_(f.ent_box)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    shares = torch.bincount(cls.reshape(-1).long(), minlength=len(CLASSES)).double() / cls.numel()
    in_view = (boxes[..., 2] >= boxes[..., 0]).any(-1).double().mean()
    vec.engine.check()
    vec.close()
    print(f"{args.env} x {n}, {args.steps} steps, {kept} kept ({kept * n} frames of {tuple(obs.shape[2:])}, labels: {args.meshes}): {dt:.2f} s")
    print("pixel shares: " + ", ".join(f"{name} {float(s):.3f}" for name, s in zip(CLASSES, shares)))
    print(f"an object in view in {float(in_view):.3f} of the kept frames")


if __name__ == "__main__":
    main()
