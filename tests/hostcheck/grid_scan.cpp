// The host path of miniworld_amd/csrc/mw_scan.h, as a program of its own (tests/test_scan_cpu.py builds it with the address and
// undefined-behaviour sanitizers): one env's map, carried through the file's calls by mwscan::scan_one.
// The file (hostcheck.h: the tokens):  the world's POSE and EXTENT;  cell gx gz shift max_range R calls;  per call: masked clear has_origin
// ox oz, then R beams t dx dz.  `shift` (0 .. 3) is the map's distance from a 4-byte boundary; every array holds exactly the elements a call
// may touch.  A call under a zero mask byte is not made (the kernel leaves such an env at once).  The answer, per call: the free plane, the
// obstacle plane, then "count0 count1 new0 new1 covered".  `grid_scan --policy N cells rays` prints mwpolicy::scan_launch.
#define HOSTCHECK_PROGRAM "grid_scan"
#include "hostcheck.h"

#include "../../miniworld_amd/csrc/mw_scan.h"
#include "../../miniworld_amd/csrc/mw_policy.h"

using namespace hostcheck;

int main(int argc, char **argv)
{
    if (argc == 5 && !strcmp(argv[1], "--policy")) {
        print_launch(mwpolicy::scan_launch(atoi(argv[2]), atoll(argv[3]), atoi(argv[4])));
        return 0;
    }
    FILE *f = argc == 2 ? fopen(argv[1], "r") : nullptr;
    if (!f) return 2;
    World w;
    if (!w.read(f, POSE | EXTENT)) return refused();
    mw_nav_params p{};
    p.cell = rd(f); p.gx = ri(f); p.gz = ri(f);
    const int shift = ri(f);; const double max_range = rd(f);
    const int R = ri(f), calls = ri(f);
    if (!mwpolicy::scan_launch(1, (long long)p.gx * p.gz, R).fits || !(max_range > 0.0)) return refused();
    const size_t cells = (size_t)p.gx * p.gz;
    std::vector<uint8_t> store(2 * cells + (size_t)shift, 0);
    uint8_t *rows = store.data() + shift;
    int32_t count[2] = {0, 0}, newly[2] = {-7, -7};
    for (int call = 0; call < calls; ++call) {
        const bool masked = ri(f) != 0, clear = ri(f) != 0, has_origin = ri(f) != 0;
        const double origin[3] = {rd(f), 0.0, rd(f)};
        std::vector<double> t((size_t)R), dir((size_t)R * 2);
        for (int b = 0; b < R; ++b) { t[b] = rd(f); dir[2 * b] = rd(f); dir[2 * b + 1] = rd(f); }
        std::vector<uint32_t> bits(2 * mwscan::plane_words((long long)cells));
        std::vector<int32_t> pre((size_t)R + 1);
        bool covered = true;
        if (masked)
            covered = mwscan::scan_one(w.ray().w, p, max_range, R, 0, has_origin ? origin : nullptr, t.data(), dir.data(), clear, bits.data(), pre.data(), rows,
                                       count, newly);
        for (int k = 0; k < 2; ++k)
            for (size_t c = 0; c < cells; ++c) printf("%d%c", (int)rows[k * cells + c], c + 1 == cells ? '\n' : ' ');
        printf("%d %d %d %d %d\n", (int)count[0], (int)count[1], (int)newly[0], (int)newly[1], covered ? 1 : 0);
    }
    fclose(f);
    return 0;
}
