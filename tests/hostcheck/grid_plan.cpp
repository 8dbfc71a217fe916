// The host path of miniworld_amd/csrc/mw_gridplan.h, as a program of its own (tests/test_grid_plan_cpu.py builds it with the address and
// undefined-behaviour sanitizers): one env's plans by mwgplan::run, over a plane staged by one worker.
// The file (hostcheck.h: the tokens):  the world's POSE and EXTENT;  cell gx gz shift flags T P stop_at radius;  fwd drift turn (the
// config's);  explicit has_step has_field has_extra has_trace;  with has_step fwd drift turn again (d_step's row);  T * P actions;
// gz * gx opaque bytes;  with has_field gz * gx field values;  with has_extra gz * gx bytes.
// `shift` (0 .. 3) is the planes' distance from a 4-byte boundary; `explicit` hands the pose over as d_pose and leaves the agent's at 0;
// every array holds exactly the elements a call may touch.  The answer: a row per plan — the bits of x, z, dir in hexadecimal and the
// five stats —, then with has_trace T * P rows of pose bits.
// `grid_plan --policy N gx gz plans` prints mwpolicy::gridplan_launch.
#define HOSTCHECK_PROGRAM "grid_plan"
#include "hostcheck.h"

#include "../../miniworld_amd/csrc/mw_gridplan.h"
#include "../../miniworld_amd/csrc/mw_policy.h"

using namespace hostcheck;

static unsigned long long bits_of(double v) { unsigned long long b; memcpy(&b, &v, 8); return b; }

int main(int argc, char **argv)
{
    if (argc == 6 && !strcmp(argv[1], "--policy")) {
        print_launch(mwpolicy::gridplan_launch(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5])));
        return 0;
    }
    FILE *f = argc == 2 ? fopen(argv[1], "r") : nullptr;
    if (!f) return 2;
    World w;
    if (!w.read(f, POSE | EXTENT)) return refused();
    mw_nav_params p{};
    p.cell = rd(f); p.gx = ri(f); p.gz = ri(f);
    const int shift = ri(f);
    mwgplan::Call q{};
    q.flags = ri(f); q.T = ri(f); q.P = ri(f); q.stop_at = ri(f); q.radius = rd(f);
    q.fwd = rd(f); q.drift = rd(f); q.turn = rd(f);
    const bool explicit_pose = ri(f), has_step = ri(f), has_field = ri(f), has_extra = ri(f), has_trace = ri(f);
    if (!mwpolicy::gridplan_launch(1, p.gx, p.gz, q.P).fits || q.T < 1 || q.T > MW_MAX_PLAN || !(q.radius >= 0.0) || q.radius > MW_GPLAN_MAX_RADIUS * p.cell ||
        (q.stop_at >= 0 && !has_field))
        return refused();
    std::vector<double> pose, step;
    if (explicit_pose) { pose = {w.ax, w.az, w.adir}; w.ax = w.az = w.adir = 0.0; }
    if (has_step) { step.resize(3); for (double &v : step) v = rd(f); }
    const size_t cells = (size_t)p.gx * p.gz, n = (size_t)q.T * q.P;
    const bool bytes = (q.flags & MW_GPLAN_BYTE_PLANS) != 0;
    std::vector<uint8_t> plans8(bytes ? n : 0), store(cells + (size_t)shift), xstore(has_extra ? cells + (size_t)shift : 0);
    std::vector<int32_t> plans32(bytes ? 0 : n);
    for (size_t k = 0; k < n; ++k) { const int a = ri(f); if (bytes) plans8[k] = (uint8_t)a; else plans32[k] = a; }
    for (size_t c = 0; c < cells; ++c) store[shift + c] = (uint8_t)ri(f);
    std::vector<uint16_t> field(has_field ? cells : 0);
    for (uint16_t &v : field) v = (uint16_t)ri(f);
    for (size_t c = 0; has_extra && c < cells; ++c) xstore[shift + c] = (uint8_t)ri(f);
    fclose(f);
    const MwRayArgs a = w.ray();
    const mwgplan::Env e = mwgplan::env_of(a.w, p, q, has_step ? step.data() : nullptr, 0);
    std::vector<uint32_t> bits((size_t)mwgplan::plane_words(p.gx, p.gz));
    if (e.covered) {
        mwgplan::zero_plane(bits.data(), p.gx, p.gz, 0, 1);
        mwgplan::stage_plane(store.data() + shift, bits.data(), p.gx, p.gz, e.outside, 0, 1, [](uint32_t *word, uint32_t bit) { *word |= bit; });
    }
    std::vector<double> pose_out((size_t)q.P * 3), trace(has_trace ? n * 3 : 0);
    std::vector<int32_t> stats((size_t)q.P * 5);
    const double x = explicit_pose ? pose[0] : a.w.ax[0], z = explicit_pose ? pose[1] : a.w.az[0], dir = explicit_pose ? pose[2] : a.adir[0];
    for (int k = 0; k < q.P; ++k)
        mwgplan::run(e, q, 1, bits.data(), bytes ? (const void *)plans8.data() : (const void *)plans32.data(), 0, (size_t)k, x, z, dir, has_field ? field.data() : nullptr,
                     has_extra ? xstore.data() + shift : nullptr, pose_out.data(), stats.data(), has_trace ? trace.data() : nullptr);
    for (int k = 0; k < q.P; ++k) {
        const double *o = pose_out.data() + 3 * k;
        const int32_t *s = stats.data() + 5 * k;
        printf("%016llx %016llx %016llx %d %d %d %d %d\n", bits_of(o[0]), bits_of(o[1]), bits_of(o[2]), (int)s[0], (int)s[1], (int)s[2], (int)s[3], (int)s[4]);
    }
    for (size_t k = 0; k < trace.size(); k += 3) printf("%016llx %016llx %016llx\n", bits_of(trace[k]), bits_of(trace[k + 1]), bits_of(trace[k + 2]));
    return 0;
}
