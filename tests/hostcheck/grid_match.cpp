// The host path of miniworld_amd/csrc/mw_match.h, as a program of its own (tests/test_match_cpu.py builds it with the address and
// undefined-behaviour sanitizers): one env's match by mwmatch::match_one.
// The file (hostcheck.h: the tokens):  the world's POSE and EXTENT;  cell gx gz shift max_range R K W has_origin quad ox oz;  K pairs c s;  R beams
// t dx dz;  gz * gx score bytes.  `shift` (0 .. 3) is the score plane's distance from a 4-byte boundary; every array holds exactly the
// elements a call may touch.  The answer: "r a b score covered", then the volume, a row per (rotation, b).
// `grid_match --policy N gz gx rays window` prints mwpolicy::match_launch, with "quad batch" behind the four.
#define HOSTCHECK_PROGRAM "grid_match"
#include "hostcheck.h"

#include "../../miniworld_amd/csrc/mw_match.h"
#include "../../miniworld_amd/csrc/mw_policy.h"

using namespace hostcheck;

int main(int argc, char **argv)
{
    if (argc == 7 && !strcmp(argv[1], "--policy")) {
        const mwpolicy::MatchLaunch l = mwpolicy::match_launch(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]));
        printf("%llu %d %zu %d %d %d\n", l.grid, l.threads, l.lds, l.fits ? 1 : 0, l.quad ? 1 : 0, l.batch);
        return 0;
    }
    FILE *f = argc == 2 ? fopen(argv[1], "r") : nullptr;
    if (!f) return 2;
    World w;
    if (!w.read(f, POSE | EXTENT)) return refused();
    mw_nav_params p{};
    p.cell = rd(f); p.gx = ri(f); p.gz = ri(f);
    const int shift = ri(f); const double max_range = rd(f);
    const int R = ri(f), K = ri(f), W = ri(f), has_origin = ri(f), quad = ri(f);
    const double origin[3] = {rd(f), 0.0, rd(f)};
    if (!mwpolicy::match_launch(1, p.gz, p.gx, R, W).fits || !(max_range > 0.0) || K < 1 || K > MW_MATCH_MAX_ROT) return refused();
    MwMatchRot rot{};
    rot.n = K;
    for (int r = 0; r < K; ++r) { rot.cs[r][0] = rd(f); rot.cs[r][1] = rd(f); }
    std::vector<double> t((size_t)R), dir((size_t)R * 2);
    for (int b = 0; b < R; ++b) { t[b] = rd(f); dir[2 * b] = rd(f); dir[2 * b + 1] = rd(f); }
    const size_t cells = (size_t)p.gx * p.gz, side = 2 * (size_t)W + 1;
    std::vector<uint8_t> store(cells + (size_t)shift), plane(mwmatch::plane_bytes((long long)cells, quad != 0));
    for (size_t c = 0; c < cells; ++c) store[shift + c] = (uint8_t)ri(f);
    fclose(f);
    std::vector<uint32_t> ends((size_t)R);
    std::vector<int32_t> volume((size_t)K * side * side, -7);
    int32_t best[3] = {-7, -7, -7}, best_score = -7;
    const bool covered = mwmatch::match_one(w.ray().w, p, max_range, R, rot, W, quad != 0, 0, has_origin ? origin : nullptr, t.data(), dir.data(), store.data() + shift,
                                            plane.data(), ends.data(), best, &best_score, volume.data());
    printf("%d %d %d %d %d\n", (int)best[0], (int)best[1], (int)best[2], (int)best_score, covered ? 1 : 0);
    for (size_t k = 0; k < volume.size(); ++k) printf("%d%c", (int)volume[k], (k + 1) % side == 0 ? '\n' : ' ');
    return 0;
}
