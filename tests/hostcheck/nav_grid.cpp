// The host path of miniworld_amd/csrc/mw_nav_grid.h, as a program of its own (tests/test_nav_grid_cpu.py builds it with the address
// and undefined-behaviour sanitizers): one env's grids from a file, the field by whole-grid passes and again by directional sweeps —
// the two must agree —, then the grid query at the file's positions.
//
// The file (hostcheck.h: the tokens):
//   cell margin reach gx gz flags shift
//   min_x min_z
//   has_target [x y z]
//   has_sources has_extra
//   gz * gx bytes of blocked, then of sources and of extra where the file has them
//   nq, then x z per position
// `shift` (0 .. 3) is the distance of every row from a 4-byte boundary: the rows of an env are not aligned when the cell count is odd,
// and each row is the last bytes of an allocation of its own, so that the sanitizer sees a read past either end.
// The answer: "field <ok> <passes> <sweep rounds>", the gz * gx cells, then "cost next wx wz" per position (%a).
//
// `nav_grid --policy N cells weighted` prints mwpolicy::nav_grid_launch instead: "grid threads lds fits"; `nav_grid --radius cell
// margin` prints mwnav::inflate_radius.
#define HOSTCHECK_PROGRAM "nav_grid"
#include "hostcheck.h"

#include "../../miniworld_amd/csrc/mw_nav_grid.h"
#include "../../miniworld_amd/csrc/mw_policy.h"

using namespace hostcheck;

namespace {

// a row of `cells` bytes that starts `shift` bytes behind a 4-byte boundary and ends with its allocation
struct Row {
    std::vector<uint8_t> store;
    uint8_t *at = nullptr;
    Row(size_t cells, int shift) : store(cells + (size_t)shift), at(store.data() + shift) {}
    void read(FILE *f, size_t cells)
    {
        for (size_t c = 0; c < cells; ++c) {
            const int v = ri(f);
            if (v < 0 || v > 255) short_file();
            at[c] = (uint8_t)v;
        }
    }
};

}  // namespace

int main(int argc, char **argv)
{
    if (argc == 5 && !strcmp(argv[1], "--policy")) {
        print_launch(mwpolicy::nav_grid_launch(atoi(argv[2]), atoll(argv[3]), atoi(argv[4]) != 0));
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "--radius")) {
        printf("%d\n", mwnav::inflate_radius(atof(argv[2]), atof(argv[3])));
        return 0;
    }
    if (argc != 2) { fprintf(stderr, "usage: nav_grid GRIDS | nav_grid --policy N cells weighted | nav_grid --radius cell margin\n"); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    mw_nav_params p{};
    p.cell = rd(f); p.margin = rd(f); p.reach = rd(f);
    p.gx = ri(f); p.gz = ri(f); p.flags = ri(f);
    const int shift = ri(f);
    double extent[4] = {0.0, 0.0, 0.0, 0.0};       // [4][N], N = 1: min_x, max_x, min_z, max_z (the maxima are not read)
    extent[0] = rd(f); extent[2] = rd(f);
    double target[3];
    const bool has_target = ri(f) != 0;
    if (has_target) for (double &v : target) v = rd(f);
    const bool has_sources = ri(f) != 0, has_extra = ri(f) != 0;
    if (!(p.cell > 0.0) || p.gx < 1 || p.gz < 1 || (long long)p.gx * p.gz > MW_NAV_MAX_CELLS || shift < 0 || shift > 3 ||
        mwnav::inflate_radius(p.cell, p.margin) < 0 || (p.flags & MW_NAV_ENTITIES) || (!has_target && !has_sources) || (has_target && !(p.reach > 0.0)))
        return refused();
    const size_t cells = (size_t)p.gx * p.gz;
    Row blocked(cells, shift), sources(has_sources ? cells : 0, shift), extra(has_extra ? cells : 0, shift);
    blocked.read(f, cells);
    if (has_sources) sources.read(f, cells);
    if (has_extra) extra.read(f, cells);
    const int nq = ri(f);
    std::vector<double> q((size_t)(nq > 0 ? nq : 0) * 2);
    for (double &v : q) v = rd(f);
    fclose(f);

    MwNavArgs a{};
    a.extent = extent;
    a.N = 1;
    std::vector<uint16_t> field(cells), swept(cells);
    std::vector<uint8_t> x(has_extra ? cells : 0);
    int passes = 0, rounds = 0;
    const double *tg = has_target ? target : nullptr;
    const uint8_t *src = has_sources ? sources.at : nullptr, *ext = has_extra ? extra.at : nullptr;
    const bool ok = mwnav::build_grid_one(a, p, blocked.at, src, tg, ext, 0, field.data(), x.data(), 0, &passes);
    const bool ok2 = mwnav::build_grid_one(a, p, blocked.at, src, tg, ext, 0, swept.data(), x.data(), 1, &rounds);
    if (ok != ok2 || field != swept) { fprintf(stderr, "nav_grid: the sweeps and the whole-grid passes disagree\n"); return 1; }
    printf("field %d %d %d\n", ok ? 1 : 0, passes, rounds);
    for (size_t c = 0; c < cells; ++c) printf("%u%c", (unsigned)field[c], c + 1 == cells ? '\n' : ' ');
    const mwnav::Grid g = mwnav::grid_of(a, p, 0);
    for (int i = 0; i < nq; ++i) {
        const mwnav::Answer r = mwnav::query_grid(g, field.data(), q[(size_t)i * 2], q[(size_t)i * 2 + 1]);
        printf("%d %d %a %a\n", (int)r.cost, (int)r.next, r.wx, r.wz);
    }
    return 0;
}
