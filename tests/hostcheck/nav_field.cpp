// The host path of miniworld_amd/csrc/mw_nav.h, as a program of its own (tests/test_nav_cpu.py builds it with the address and
// undefined-behaviour sanitizers): one env's world from a file, the field by whole-grid passes and again by directional sweeps — the
// two must agree —, then the query at the file's positions.
//
// The file (hostcheck.h: the tokens, the world block):
//   cell margin reach gx gz flags target_slot
//   the world: AGENT with CARRY, EXTENT, SEGS, SLOTS
//   has_target [x y z]
//   nq, then x z per position
// The answer: "field <ok> <passes> <sweep rounds>", the gz * gx cells, then "cost next wx wz" per position (%a).
#define HOSTCHECK_PROGRAM "nav_field"
#include "hostcheck.h"

#include "../../miniworld_amd/csrc/mw_nav.h"

using namespace hostcheck;

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: nav_field WORLD\n"); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    mw_nav_params p{};
    p.cell = rd(f); p.margin = rd(f); p.reach = rd(f);
    p.gx = ri(f); p.gz = ri(f); p.flags = ri(f); p.target_slot = ri(f);
    World world;
    if (!world.read(f, AGENT | CARRY | EXTENT | SEGS | SLOTS)) return refused();
    const int E = world.E;
    double target[3];
    const bool has_target = ri(f) != 0;
    if (has_target) for (double &v : target) v = rd(f);
    const int nq = ri(f);
    std::vector<double> q((size_t)(nq > 0 ? nq : 0) * 2);
    for (double &v : q) v = rd(f);
    fclose(f);
    if (p.gx < 1 || p.gz < 1 || (long long)p.gx * p.gz > MW_NAV_MAX_CELLS || p.target_slot < 0 || p.target_slot >= (E > 0 ? E : 1))
        return refused();
    const MwNavArgs a = world.nav();

    const size_t cells = (size_t)p.gx * p.gz;
    std::vector<uint16_t> field(cells), swept(cells);
    int passes = 0, rounds = 0;
    const double *tg = has_target ? target : nullptr;
    const bool ok = mwnav::build_one(a, p, tg, 0, field.data(), 0, &passes);
    const bool ok2 = mwnav::build_one(a, p, tg, 0, swept.data(), 1, &rounds);
    if (ok != ok2 || field != swept) { fprintf(stderr, "nav_field: the sweeps and the whole-grid passes disagree\n"); return 1; }
    printf("field %d %d %d\n", ok ? 1 : 0, passes, rounds);
    for (size_t c = 0; c < cells; ++c) printf("%u%c", (unsigned)field[c], c + 1 == cells ? '\n' : ' ');
    const mwnav::Grid g = mwnav::grid_of(a, p, 0);
    const mwnav::Target t = mwnav::target_of(a, p, tg, 0);
    for (int i = 0; i < nq; ++i) {
        const mwnav::Answer r = mwnav::query(g, field.data(), t, q[(size_t)i * 2], q[(size_t)i * 2 + 1]);
        printf("%d %d %a %a\n", (int)r.cost, (int)r.next, r.wx, r.wz);
    }
    return 0;
}
