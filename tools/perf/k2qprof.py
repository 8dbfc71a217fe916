"""Timeline of the quad raster kernel (mw_rasterq.hip) from a perf build (make EXTRA=-DMW_PERF_HOOKS): s_memtime stamps of every
wavefront at the phase boundaries, and of every workgroup of the launch — the ones that leave early too — at its first instruction
and its last wavefront's exit, with its kind (drawn, clean, copied, idle).
usage (GPU box): python tools/perf/k2qprof.py [config] [steps]   (runs a bench with MW_K2Q_PROF set and summarises the dump of its
last step; steps: enough for the frame cache to reach its steady shares, default 400)
       (anywhere): python tools/perf/k2qprof.py --dump=FILE         (summarises the dump of an earlier run)"""
import os, subprocess, sys, tempfile
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = [a for a in sys.argv[1:] if not a.startswith("--dump=")]
dumps = [a[7:] for a in sys.argv[1:] if a.startswith("--dump=")]
cfg = args[0] if args else "hallway"
steps = int(args[1]) if len(args) > 1 else 400
if dumps:           # an earlier run's dump (MW_K2Q_PROF=<file> python bench.py ...): summarise it, run nothing
    dump = dumps[0]
else:
    dump = os.path.join(tempfile.mkdtemp(), "k2qprof.bin")
    env = dict(os.environ, MW_K2Q_PROF=dump)
    subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", cfg, "--steps", str(steps), "--warmup", "4"], env=env, check=True,
                   stdout=subprocess.DEVNULL)
raw = np.fromfile(dump, np.uint64)
n_env = raw.size // 96
t = raw[:n_env * 64].reshape(-1, 8, 8).astype(np.int64)      # [env][wave][stamp]: s_memtime, the shader clock of the env's XCD
cls = raw[n_env * 64:n_env * 80].reshape(n_env, 16)[:, :9].astype(np.int64)
wg = raw[n_env * 80:].reshape(n_env, 16).astype(np.int64)    # [workgroup]: start, kind, the wavefronts' exits: s_memrealtime, 100 MHz, one clock for all XCDs; [10] env, [11] its list length (plan_order_sim.py)
TICKS = 100.0       # s_memrealtime ticks per us

# ---- every workgroup of the launch, by blockIdx
KINDS = ["drawn", "clean", "copied", "idle"]
start, end, kind = wg[:, 0] / TICKS, wg[:, 2:10].max(axis=1) / TICKS, wg[:, 1]
seen = wg[:, 0] > 0
if not seen.any():
    sys.exit("no workgroup stamps in the dump: the library is not a perf build")
t0 = start[seen].min()
start, end = start - t0, end - t0
k_end = end[seen].max()
if k_end > 5000.0:
    sys.exit(f"the stamps span {k_end:.0f} us: not one launch of this kernel")
print(f"workgroups {int(seen.sum())} of {n_env}; launch span (first start to last exit) {k_end:.1f} us")
print("kind      count  share   residency us: mean / median / p95     sum of residencies / span")
for k, name in enumerate(KINDS):
    m = seen & (kind == k)
    if not m.any():
        continue
    r = end[m] - start[m]
    print(f"  {name:7s} {int(m.sum()):5d}  {100.0 * m.sum() / seen.sum():5.1f}%   {r.mean():7.2f} / {np.median(r):7.2f} / {np.percentile(r, 95):7.2f}      {r.sum() / k_end:7.1f}")
drawn = seen & (kind == 0)
print("resident workgroups in 5 us bins (mean over the bin): t us | drawn | not drawn")
for lo in np.arange(0.0, k_end, 5.0):
    hi = lo + 5.0
    ov = np.clip(np.minimum(end, hi) - np.maximum(start, lo), 0.0, None) / 5.0
    print(f"  {lo:6.0f}  {ov[drawn].sum():7.1f}  {ov[seen & ~drawn].sum():7.1f}")
if drawn.any():
    last = start[drawn].max()
    print(f"last drawing workgroup starts at {last:.1f} us, the launch ends at {k_end:.1f}: tail {k_end - last:.1f} us")
    starts = np.sort(start[drawn])
    print("drawing workgroups started by 25 / 50 / 75 / 100 % of the span: " + " / ".join(str(int((starts <= f * k_end).sum())) for f in (0.25, 0.5, 0.75, 1.0)))
    print(f"sum of the drawing workgroups' residencies {(end[drawn] - start[drawn]).sum() / 1000.0:.1f} ms; of the others' {(end[seen & ~drawn] - start[seen & ~drawn]).sum() / 1000.0:.2f} ms")

# ---- the drawing workgroups' phases (by env; shader-clock ticks, scaled by the drawing workgroups' median residency)
life = t[:, :, 7].max(axis=1) - t[:, :, 0].min(axis=1)
live = (t[:, :, 0].min(axis=1) > 0) & (life > 0) & (life < np.median(life[life > 0]) * 20)      # (an env's stamps are its last drawing's; other XCD, other origin: no way to tell the step)
t = t[live]
print('quads per class, mean per env over its last drawing (FALLBACK BIG EXACT P4 P3 P2 P1 TRIV SKY):', np.round(cls[live].mean(axis=0), 1).tolist())
names = ["stage", "A tiles", "B quads", "C classes", "D batches", "wait", "D2 exact", "E(rgb)"]
d = np.diff(t, axis=2)
med_life = np.median(life[live])
print(f"per-wave phase durations, % of the median block lifetime ({med_life:.0f} shader-clock ticks, first stamp to last E start): median / mean / p95 over wavefronts")
for k in range(7):
    v = d[:, :, k].reshape(-1) * 100.0 / med_life
    print(f"  {names[k]:10s} {np.median(v):7.2f} {v.mean():7.2f} {np.percentile(v, 95):7.2f}")
