// The host path of miniworld_amd/csrc/mw_nav.h, as a program of its own (tests/test_nav_cpu.py builds it with the address and
// undefined-behaviour sanitizers): one env's world from a file, the field by whole-grid passes and again by directional sweeps — the
// two must agree —, then the query at the file's positions.
//
// The file, whitespace-separated (doubles as Python's repr, which round-trips):
//   cell margin reach gx gz flags target_slot
//   agent_radius max_forward_step carry
//   min_x max_x min_z max_z
//   nsegs, then ax az bx bz per segment
//   E, then kind x y z radius per slot
//   has_target [x y z]
//   nq, then x z per position
// The answer: "field <ok> <passes> <sweep rounds>", the gz * gx cells, then "cost next wx wz" per position (%a).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../miniworld_amd/csrc/mw_nav.h"

static double rd(FILE *f)
{
    double v;
    if (fscanf(f, "%lf", &v) != 1) { fprintf(stderr, "nav_field: short file\n"); exit(2); }
    return v;
}
static int ri(FILE *f)
{
    int v;
    if (fscanf(f, "%d", &v) != 1) { fprintf(stderr, "nav_field: short file\n"); exit(2); }
    return v;
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: nav_field WORLD\n"); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    mw_nav_params p{};
    p.cell = rd(f); p.margin = rd(f); p.reach = rd(f);
    p.gx = ri(f); p.gz = ri(f); p.flags = ri(f); p.target_slot = ri(f);
    MwNavArgs a{};
    a.agent_radius = rd(f); a.max_forward_step = rd(f);
    int32_t carry = ri(f);
    std::vector<double> extent(4);
    for (double &v : extent) v = rd(f);
    int32_t nsegs = ri(f);
    std::vector<double> segs((size_t)nsegs * 4 + 1);
    for (int i = 0; i < nsegs * 4; ++i) segs[i] = rd(f);
    const int E = ri(f);
    std::vector<int32_t> kind((size_t)E + 1);
    std::vector<double> pos((size_t)E * 3 + 1), geom((size_t)E * 9 + 1);
    for (int s = 0; s < E; ++s) {       // (the engine's layouts with N = 1: [3][E], [9][E])
        kind[s] = ri(f);
        for (int k = 0; k < 3; ++k) pos[(size_t)k * E + s] = rd(f);
        geom[(size_t)7 * E + s] = rd(f);
    }
    double target[3];
    const bool has_target = ri(f) != 0;
    if (has_target) for (double &v : target) v = rd(f);
    const int nq = ri(f);
    std::vector<double> q((size_t)nq * 2 + 1);
    for (int i = 0; i < nq * 2; ++i) q[i] = rd(f);
    fclose(f);
    if (p.gx < 1 || p.gz < 1 || (long long)p.gx * p.gz > MW_NAV_MAX_CELLS || p.target_slot < 0 || p.target_slot >= (E > 0 ? E : 1)) {
        fprintf(stderr, "nav_field: parameters the engine refuses\n");
        return 2;
    }
    uint32_t status = 0;
    a.segs = segs.data(); a.nsegs = &nsegs; a.extent = extent.data(); a.ekind = kind.data(); a.epos = pos.data(); a.egeom = geom.data();
    a.carry = &carry; a.ax = nullptr; a.az = nullptr; a.status = &status;
    a.N = 1; a.E = E; a.max_segs = nsegs; a.shared_geom = 1;

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
