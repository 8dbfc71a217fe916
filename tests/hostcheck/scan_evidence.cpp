// The host path of miniworld_amd/csrc/mw_evidence.h, as a program of its own (tests/test_scan_evidence_cpu.py builds it with the address
// and undefined-behaviour sanitizers): one env's evidence, carried through the file's calls by mwevid::evidence_one.
// The file (hostcheck.h: the tokens):  the world's POSE and EXTENT;  cell gx gz shift max_range R calls first;  per call: masked clear
// has_origin ox oz, hit miss cap lo hi free_at occ_at, outputs (1: map, 2: score, 4: changed), then R beams t dx dz.  `shift` (0 .. 3) is
// the evidence row's distance from a 4-byte boundary, the map's is shift + 1 and the score's shift + 2; every array holds exactly the
// elements a call may touch.  `first`: 1, or 0 for the form that deals the start cell as a task.  A call under a zero mask byte is not
// made (the kernel leaves such an env at once).  The answer, per call: ev, the free plane, the obstacle plane, the score plane (a plane
// not asked for stays as it was), then "count0 count1 changed0 changed1 covered".  `scan_evidence --policy N cells rays` prints
// mwpolicy::evidence_launch.
#define HOSTCHECK_PROGRAM "scan_evidence"
#include "hostcheck.h"

#include "../../miniworld_amd/csrc/mw_evidence.h"
#include "../../miniworld_amd/csrc/mw_policy.h"

using namespace hostcheck;

int main(int argc, char **argv)
{
    if (argc == 5 && !strcmp(argv[1], "--policy")) {
        print_launch(mwpolicy::evidence_launch(atoi(argv[2]), atoll(argv[3]), atoi(argv[4])));
        return 0;
    }
    FILE *f = argc == 2 ? fopen(argv[1], "r") : nullptr;
    if (!f) return 2;
    World w;
    if (!w.read(f, POSE | EXTENT)) return refused();
    mw_nav_params p{};
    p.cell = rd(f); p.gx = ri(f); p.gz = ri(f);
    const int shift = ri(f);
    const double max_range = rd(f);
    const int R = ri(f), calls = ri(f), first = ri(f);
    if (!mwpolicy::evidence_launch(1, (long long)p.gx * p.gz, R).fits || !(max_range > 0.0)) return refused();
    const size_t cells = (size_t)p.gx * p.gz;
    const int map_shift = (shift + 1) & 3, score_shift = (shift + 2) & 3;
    std::vector<int8_t> ev_store(cells + (size_t)shift, 0);
    std::vector<uint8_t> map_store(2 * cells + (size_t)map_shift, 0), score_store(cells + (size_t)score_shift, 0);
    int8_t *ev = ev_store.data() + shift;
    uint8_t *map = map_store.data() + map_shift, *score = score_store.data() + score_shift;
    int32_t count[2] = {0, 0}, changed[2] = {-7, -7};
    for (int call = 0; call < calls; ++call) {
        const bool masked = ri(f) != 0, clear = ri(f) != 0, has_origin = ri(f) != 0;
        const double origin[3] = {rd(f), 0.0, rd(f)};
        mwevid::Rule r{};
        r.hit = ri(f); r.miss = ri(f); r.cap = ri(f); r.lo = ri(f); r.hi = ri(f); r.free_at = ri(f); r.occ_at = ri(f);
        const int outputs = ri(f);
        if (mwevid::out_of_range(r)) return refused();
        std::vector<double> t((size_t)R), dir((size_t)R * 2);
        for (int b = 0; b < R; ++b) { t[b] = rd(f); dir[2 * b] = rd(f); dir[2 * b + 1] = rd(f); }
        std::vector<uint32_t> cnt(cells);
        std::vector<int32_t> pre((size_t)R + 1);
        bool covered = true;
        if (masked)
            covered = mwevid::evidence_one(w.ray().w, p, max_range, R, 0, has_origin ? origin : nullptr, t.data(), dir.data(), clear, r, first, cnt.data(), pre.data(), ev,
                                           outputs & 1 ? map : nullptr, outputs & 2 ? score : nullptr, count, outputs & 4 ? changed : nullptr);
        for (size_t c = 0; c < cells; ++c) printf("%d%c", (int)ev[c], c + 1 == cells ? '\n' : ' ');
        for (int k = 0; k < 2; ++k)
            for (size_t c = 0; c < cells; ++c) printf("%d%c", (int)map[k * cells + c], c + 1 == cells ? '\n' : ' ');
        for (size_t c = 0; c < cells; ++c) printf("%d%c", (int)score[c], c + 1 == cells ? '\n' : ' ');
        printf("%d %d %d %d %d\n", (int)count[0], (int)count[1], (int)changed[0], (int)changed[1], covered ? 1 : 0);
    }
    fclose(f);
    return 0;
}
