// The host path of miniworld_amd/csrc/mw_search.h under sanitizers (tests/test_search_cpu.py): one env's search by mwsearch::search_one.
// The file: grid_match.cpp's without its form.  The answer: "r a b score covered refined blocks" with pruning on, the same with pruning
// off, then the bounds, a row of blocks per rotation (block q = j * side + i is anchored at (-W + 8 j, -W + 8 i)).
// `grid_search --policy N gz gx rays window` prints mwpolicy::search_launch, with "batch" behind the four.
#define HOSTCHECK_PROGRAM "grid_search"
#include "hostcheck.h"
#include "../../miniworld_amd/csrc/mw_search.h"
#include "../../miniworld_amd/csrc/mw_policy.h"
using namespace hostcheck;

int main(int argc, char **argv)
{
    if (argc == 7 && !strcmp(argv[1], "--policy")) {
        const mwpolicy::SearchLaunch l = mwpolicy::search_launch(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]));
        printf("%llu %d %zu %d %d\n", l.grid, l.threads, l.lds, l.fits ? 1 : 0, l.batch);
        return 0;
    }
    FILE *f = argc == 2 ? fopen(argv[1], "r") : nullptr;
    if (!f) return 2;
    World w;
    if (!w.read(f, POSE | EXTENT)) return refused();
    mw_nav_params p{};
    p.cell = rd(f); p.gx = ri(f); p.gz = ri(f);
    const int shift = ri(f); const double max_range = rd(f);
    const int R = ri(f), K = ri(f), W = ri(f), has_origin = ri(f);
    const double origin[3] = {rd(f), 0.0, rd(f)};
    if (!mwpolicy::search_launch(1, p.gz, p.gx, R, W).fits || !(max_range > 0.0) || K < 1 || K > MW_MATCH_MAX_ROT) return refused();
    MwMatchRot rot{};
    rot.n = K;
    for (int r = 0; r < K; ++r) { rot.cs[r][0] = rd(f); rot.cs[r][1] = rd(f); }
    std::vector<double> t((size_t)R), dir((size_t)R * 2);
    for (int b = 0; b < R; ++b) { t[b] = rd(f); dir[2 * b] = rd(f); dir[2 * b + 1] = rd(f); }
    const size_t cells = (size_t)p.gx * p.gz, nblk = (size_t)mwsearch::blocks(W);
    std::vector<uint8_t> store(cells + (size_t)shift), plane(mwsearch::plane_bytes((long long)cells)), M(mwsearch::bound_bytes(p.gz, p.gx));
    for (size_t c = 0; c < cells; ++c) store[shift + c] = (uint8_t)ri(f);
    fclose(f);
    std::vector<uint32_t> ends((size_t)R), words(nblk);
    const double *o = has_origin ? origin : nullptr;
    for (int prune = 1; prune >= 0; --prune) {
        int32_t best[3] = {-7, -7, -7}, best_score = -7, stats[2] = {-7, -7};
        const bool covered = mwsearch::search_one(w.ray().w, p, max_range, R, rot, W, prune != 0, 0, o, t.data(), dir.data(), store.data() + shift, plane.data(),
                                                  M.data(), ends.data(), words.data(), best, &best_score, stats);
        printf("%d %d %d %d %d %d %d\n", (int)best[0], (int)best[1], (int)best[2], (int)best_score, covered ? 1 : 0, (int)stats[0], (int)stats[1]);
        if (!covered) return 0;
    }
    // the bounds alone: the phases of search_one up to them (the planes stand from the runs above)
    const mwnav::Grid g = mwnav::grid_of(w.ray().w, p, 0);
    const mwmatch::Match m{g, o ? o[0] : w.ray().w.ax[0], o ? o[2] : w.ray().w.az[0], max_range, t.data(), dir.data(), R, W};
    for (int r = 0; r < K; ++r) {
        uint32_t fill[MW_MATCH_MAX_ROT] = {};
        mwmatch::list_ends(m, rot.cs[r][0], rot.cs[r][1], ends.data(), fill + r, 0, 1);
        mwsearch::bound_blocks(M.data(), g.gx, g.gz, W, r, 1, ends.data(), R, fill, words.data(), 0, 1);
        for (size_t k = 0; k < nblk; ++k) printf("%u%c", words[k], k + 1 == nblk ? '\n' : ' ');
    }
    return 0;
}
