"""What ordering the quad kernel's draw list by a predicted cost would save: joins every drawing workgroup's residency in a perf
build's dump (make EXTRA=-DMW_PERF_HOOKS; the stamps of tools/perf/k2qprof.py, with the env and its display-list length in words 10
and 11 of a workgroup's row, and the env's class sizes of the drawing before this one in words 9..11 of its class row) with the
candidate predictors, and prints
  (a) the Spearman rank correlation of each predictor with the residency,
  (b) least-squares weights of the residency on the class sizes and the partial events,
  (c) a list-scheduling simulation on 768 slots (3 workgroups x 256 CUs) with the measured residencies as job lengths: the order as
      dispatched, by true residency (the oracle), and by each predictor, unquantised and in B = 2, 4, 8, 16 classes.
The simulation knows nothing of workgroups that run faster in an emptier chip: where its as-dispatched span misses the measured one
its savings are upper estimates.
usage (GPU box): python tools/perf/plan_order_sim.py [config] [steps]     (a bench with MW_K2Q_PROF set, the dump of its last step)
       (anywhere): python tools/perf/plan_order_sim.py --dump=FILE [--weights=w0,..,w8] [--lo=L --hi=H]
--weights: FALLBACK BIG EXACT P4 P3 P2 P1 TRIV and the partial events, as mw_frame_plan.h keeps them (default: this dump's own fit,
scaled and rounded); --lo / --hi: the hint values the lowest and the highest class end and begin at (default: this dump's 2nd and
98th percentile)."""
import heapq, os, subprocess, sys, tempfile
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
opts = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--"))
args = [a for a in sys.argv[1:] if not a.startswith("--")]
cfg = args[0] if args else "hallway"
steps = int(args[1]) if len(args) > 1 else 400
if "dump" in opts:
    dump = opts["dump"]
else:
    dump = os.path.join(tempfile.mkdtemp(), "k2qprof.bin")
    subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", cfg, "--steps", str(steps), "--warmup", "4"],
                   env=dict(os.environ, MW_K2Q_PROF=dump), check=True, stdout=subprocess.DEVNULL)
SLOTS, TICKS = 768, 100.0
NAMES = ["FALLBACK", "BIG", "EXACT", "P4", "P3", "P2", "P1", "TRIV", "partial"]
raw = np.fromfile(dump, np.uint64)
N = raw.size // 96
cls = raw[N * 64:N * 80].reshape(N, 16)
wg = raw[N * 80:].reshape(N, 16).astype(np.int64)
seen = wg[:, 0] > 0
if not seen.any():
    sys.exit("no workgroup stamps in the dump: the library is not a perf build")
start, end, kind = wg[:, 0] / TICKS, wg[:, 2:10].max(axis=1) / TICKS, wg[:, 1]
t0 = start[seen].min()
span = end[seen].max() - t0
res = end - start
drawn = np.flatnonzero(seen & (kind == 0))          # in dispatch order
other = np.flatnonzero(seen & (kind != 0))
env, nvis = wg[drawn, 10], wg[drawn, 11].astype(np.float64)
if len(set(env.tolist())) != drawn.size:
    sys.exit("the drawing workgroups' envs are not distinct: the dump lacks words 10 and 11 (an older perf build)")
r = res[drawn]
cur = np.concatenate([cls[env, :8], cls[env, 12:13]], axis=1).astype(np.float64)         # this drawing's class sizes and partial events
pk = cls[env, 9:12]
prev = np.stack([(pk[:, c >> 2] >> np.uint64(16 * (c & 3))) & np.uint64(0xFFFF) for c in range(8)] + [(pk[:, 2] >> np.uint64(16)) & np.uint64(0xFFFF)], axis=1).astype(np.float64)
print(f"{dump}: {drawn.size} drawing workgroups of {int(seen.sum())}, residency mean {r.mean():.2f} median {np.median(r):.2f} p95 {np.percentile(r, 95):.2f} us; "
      f"envs never drawn before {(prev.sum(axis=1) == 0).sum()}")


def ranks(x):
    _, inv, cnt = np.unique(x, return_inverse=True, return_counts=True)      # ties: the mean rank
    return (np.cumsum(cnt) - (cnt + 1) / 2.0)[inv]


def spearman(x, y):
    return float(np.corrcoef(ranks(x), ranks(y))[0, 1])


# ---- (b) least squares of the residency on this drawing's class sizes and partial events
A = np.concatenate([cur, np.ones((r.size, 1))], axis=1)
w, *_ = np.linalg.lstsq(A, r, rcond=None)
fit = A @ w
print("(b) least squares, us per quad of the class / per partial event, and the intercept:")
print("    " + "  ".join(f"{n} {v:.4f}" for n, v in zip(NAMES + ["1"], w)))
print(f"    R^2 {1.0 - ((r - fit) ** 2).sum() / ((r - r.mean()) ** 2).sum():.3f}, residual rms {np.sqrt(((r - fit) ** 2).mean()):.2f} us")
if "weights" in opts:
    wi = np.array([int(v) for v in opts["weights"].split(",")], np.float64)
else:
    wi = np.round(np.clip(w[:9], 0.0, None) * 16.0 / max(w[7], 1e-9))       # in units of a sixteenth of a TRIV quad
print("    integer weights: " + ",".join(str(int(v)) for v in wi))
hint_now = np.minimum(cur @ wi, 65535.0)
hint = np.minimum(prev @ wi, 65535.0)           # what the plan kernel would have read: the hint of the drawing before this one
A3 = np.stack([nvis, hint, np.ones(r.size)], axis=1)
w3, *_ = np.linalg.lstsq(A3[hint > 0], r[hint > 0], rcond=None)
both = A3 @ w3
preds = {"P1 nvis": nvis, "P2 hint (last drawing)": hint, "P3 nvis + hint": both, "(this drawing's own hint)": hint_now}

# ---- (a)
print("(a) Spearman rank correlation with the residency:")
for n, x in preds.items():
    print(f"    {n:28s} {spearman(x, r):6.3f}")
for c in range(9):
    print(f"    {'this drawing ' + NAMES[c]:28s} {spearman(cur[:, c], r):6.3f}")


# ---- (c)
def simulate(order):
    """the drawing workgroups in `order`, then the others as dispatched, each into the slot that frees first"""
    free = [0.0] * SLOTS
    last = 0.0
    for L in np.concatenate([r[order], res[other]]):
        t = heapq.heappop(free)
        heapq.heappush(free, t + L)
        last = max(last, t + L)
    return last


def classes(x, B, lo, hi):
    return np.clip(np.floor((x - lo) * B / max(hi - lo, 1e-9)), 0, B - 1).astype(np.int64)


ident = np.arange(r.size)
s_disp, s_orc = simulate(ident), simulate(np.argsort(-r, kind="stable"))
print(f"(c) list scheduling on {SLOTS} slots: measured span {span:.1f} us; as dispatched {s_disp:.1f}; oracle {s_orc:.1f} (saves {s_disp - s_orc:.1f}); "
      f"sum of residencies / slots {(r.sum() + res[other].sum()) / SLOTS:.1f}")
if abs(s_disp - span) > 4.0:
    print(f"    the as-dispatched simulation misses the measured span by {s_disp - span:+.1f} us: the model lacks something (workgroups run faster in an "
          "emptier chip, slots are per CU), the savings below are upper estimates")
# (the measured lengths carry their place in this launch: a workgroup that ran in the emptying chip of the tail was resident for less
# time than under full load, so the order as dispatched already ends on jobs that look short.  The same lengths in random orders say
# what an order that knows nothing costs.)
rng = np.random.default_rng(0)
s_rnd = [simulate(rng.permutation(r.size)) for _ in range(8)]
print(f"    in a random order, 8 shuffles: mean {np.mean(s_rnd):.1f} (min {np.min(s_rnd):.1f}, max {np.max(s_rnd):.1f}); against that mean the oracle saves {np.mean(s_rnd) - s_orc:.1f}")
print("    predictor                      unquantised " + " ".join(f"   B={B:<2d}" for B in (2, 4, 8, 16)) + "   share of the oracle's saving (unquantised)     lo / hi")
for n, x in preds.items():
    lo = float(opts["lo"]) if "lo" in opts and n.startswith("P2") else float(np.percentile(x, 2))
    hi = float(opts["hi"]) if "hi" in opts and n.startswith("P2") else float(np.percentile(x, 98))
    s_u = simulate(np.argsort(-x, kind="stable"))
    qs = [simulate(np.argsort(-classes(x, B, lo, hi), kind="stable")) for B in (2, 4, 8, 16)]
    share = lambda base: f"{100.0 * (base - s_u) / (base - s_orc):5.0f} %" if base - s_orc > 0.5 else "    - "
    print(f"    {n:28s} {s_u:9.1f}    " + " ".join(f"{q:7.1f}" for q in qs) + f"   {share(s_disp)} (against the random orders' mean {share(float(np.mean(s_rnd)))})      {lo:.0f} / {hi:.0f}")
    if n.startswith("P1"):       # fixed class functions of the length, as mw_frame_plan.h can keep them (mw_plan_cost_class: the B = 8 one)
        for B, sh in ((4, 3), (8, 2), (16, 1)):
            c = np.minimum(B - 1, x.astype(np.int64) >> sh)
            print(f"      min({B - 1}, nvis >> {sh}): {simulate(np.argsort(-c, kind='stable')):.1f}; envs per class, cheapest first: {np.bincount(c, minlength=B).tolist()}")
    if n.startswith("P2"):
        for B in (2, 4, 8, 16):
            print(f"      B={B}: envs per class, cheapest first: {np.bincount(classes(x, B, lo, hi), minlength=B).tolist()}")
