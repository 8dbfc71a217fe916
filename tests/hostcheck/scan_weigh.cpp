// The host paths of miniworld_amd/csrc/mw_weigh.h, as a program of its own (tests/test_scan_weigh_cpu.py builds it with the address and
// undefined-behaviour sanitizers).  The file (hostcheck.h: the tokens) starts with the mode; every array holds exactly what a call may touch.
//   0  mwweigh::weigh_one: the world's POSE and EXTENT;  cell gx gz shift max_range R P waves;  R beams t dx dz;  P poses x z c s;  gz * gx
//      score bytes, `shift` (0 .. 3) from a 4-byte boundary.  The answer: "score inside" per particle, then "p score covered".
//   1  mwweigh::resample_one: P stride offset;  P weights.  Pose row p is 4 p .. 4 p + 3.  The answer: "ancestor pose_out[0]" per particle.
// `--policy N gz gx rays particles forced` prints mwpolicy::weigh_launch with "waves" behind the four, `--policy N particles` resample_launch.
#define HOSTCHECK_PROGRAM "scan_weigh"
#include "hostcheck.h"

#include "../../miniworld_amd/csrc/mw_weigh.h"
#include "../../miniworld_amd/csrc/mw_policy.h"

using namespace hostcheck;

static unsigned long long ru(FILE *f)
{
    unsigned long long v;
    if (fscanf(f, "%llu", &v) != 1) short_file();
    return v;
}

static int weigh(FILE *f)
{
    World w;
    if (!w.read(f, POSE | EXTENT)) return refused();
    mw_nav_params p{};
    p.cell = rd(f); p.gx = ri(f); p.gz = ri(f);
    const int shift = ri(f); const double max_range = rd(f);
    const int R = ri(f), P = ri(f), waves = ri(f);
    if (!mwpolicy::weigh_launch(1, (long long)p.gx * p.gz, R, P).fits || !(max_range > 0.0)) return refused();
    std::vector<double> t((size_t)R), dir((size_t)R * 2), pose((size_t)P * 4), beams((size_t)R * 3);
    for (int b = 0; b < R; ++b) { t[b] = rd(f); dir[2 * b] = rd(f); dir[2 * b + 1] = rd(f); }
    for (double &v : pose) v = rd(f);
    const size_t cells = (size_t)p.gx * p.gz;
    std::vector<uint8_t> store(cells + (size_t)shift), plane(mwweigh::plane_bytes((long long)cells));
    for (size_t c = 0; c < cells; ++c) store[shift + c] = (uint8_t)ri(f);
    std::vector<int32_t> out((size_t)P, -7), inside((size_t)P, -7);
    int32_t best[2] = {-7, -7};
    const bool covered = mwweigh::weigh_one(w.ray().w, p, max_range, R, P, waves != 0, 0, t.data(), dir.data(), store.data() + shift, pose.data(), plane.data(),
                                            beams.data(), out.data(), inside.data(), best);
    for (int q = 0; q < P; ++q) printf("%d %d\n", (int)out[q], (int)inside[q]);
    printf("%d %d %d\n", (int)best[0], (int)best[1], covered ? 1 : 0);
    return 0;
}

static int resample(FILE *f)
{
    const int P = ri(f), stride = ri(f);
    const uint64_t offset = ru(f);
    if (!mwpolicy::resample_launch(1, P).fits || stride < 1) return refused();
    std::vector<uint32_t> weight((size_t)P);
    for (uint32_t &v : weight) v = (uint32_t)ru(f);
    std::vector<uint64_t> prefix((size_t)P);
    std::vector<int32_t> ancestor((size_t)P, -7);
    std::vector<double> pose((size_t)P * 4), pose_out((size_t)P * 4, -7.0);
    for (size_t k = 0; k < pose.size(); ++k) pose[k] = (double)k;
    mwweigh::resample_one(P, stride, weight.data(), offset, prefix.data(), ancestor.data(), pose.data(), pose_out.data());
    for (int j = 0; j < P; ++j) {
        for (int k = 1; k < 4; ++k)
            if (pose_out[4 * (size_t)j + k] != pose_out[4 * (size_t)j] + k) return 3;      // (a row travels whole)
        printf("%d %d\n", (int)ancestor[j], (int)pose_out[4 * (size_t)j]);
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 8 && !strcmp(argv[1], "--policy")) {
        const mwpolicy::WeighLaunch l = mwpolicy::weigh_launch(atoi(argv[2]), (long long)atoi(argv[3]) * atoi(argv[4]), atoi(argv[5]), atoi(argv[6]), atoi(argv[7]));
        printf("%llu %d %zu %d %d\n", l.grid, l.threads, l.lds, l.fits ? 1 : 0, l.waves ? 1 : 0);
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "--policy")) {
        print_launch(mwpolicy::resample_launch(atoi(argv[2]), atoi(argv[3])));
        return 0;
    }
    FILE *f = argc == 2 ? fopen(argv[1], "r") : nullptr;
    if (!f) return 2;
    const int rc = ri(f) == 0 ? weigh(f) : resample(f);
    fclose(f);
    return rc;
}
