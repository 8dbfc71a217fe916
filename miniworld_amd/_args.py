"""The argument rules of the batched env (vec_env.py and its mixins), one helper per rule: a real number, an integer, seeds, and
whether a snapshot is on a device.  A refusal is a ValueError that names the method and the argument, raised before anything is
launched; none of them touches the engine.  The two rules that need the env's device — a tensor of a shape and dtype there
(_is_tensor), a uint8 / bool mask there (_device_mask) — are methods of MiniWorldVecEnv."""
from __future__ import annotations

import math

import numpy as np


INF = math.inf


def real(where, name, v, lo=0.0, hi=INF, lo_open=True):
    """`v` as a float: a real number — Python's or numpy's, never a bool —, finite, lo < v <= hi (lo_open=False: lo <= v).  (Plain
    comparisons and no call, for the calls that check scalars on every use: the bounds refuse a NaN.)"""
    if (isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating))
            or not ((lo < v if lo_open else lo <= v) and v <= hi and v != INF)):
        raise ValueError(f"{where}: {name} {v!r} must be a finite number {'>' if lo_open else '>='} {lo:g}" + (f" and <= {hi:g}" if hi < INF else ""))
    return float(v)


def integer(where, name, v, lo, hi):
    """`v` as an int: an integer — Python's or numpy's, never a bool — in lo .. hi"""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
        raise ValueError(f"{where}: {name} must be an integer in {lo} .. {hi}, not {v!r}")
    return int(v)


def seeds_u64(where, seeds, below=2 ** 64):
    """the integers `seeds` (a host sequence or array) as a numpy uint64 array, every one in 0 .. below - 1 — the device reads a seed's
    bits as uint64, so a negative one would become a huge one without a word.  (Python integers meanwhile: seeds up to 2^64 - 1 keep
    their bits.)"""
    vals = [int(x) for x in np.asarray(seeds, dtype=object).ravel()]
    if any(not 0 <= x < below for x in vals):
        raise ValueError(f"{where}: seeds: need non-negative integers below 2^{(below - 1).bit_length()}")
    return np.array(vals, dtype=np.uint64)


def on_device(snap, device):
    """whether the buffers of the EnvSnapshot `snap` are on `device`"""
    return snap.data.device == device and (snap.frames is None or snap.frames.device == device)
