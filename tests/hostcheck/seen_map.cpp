// The host path of miniworld_amd/csrc/mw_seen.h, as a program of its own (tests/test_seen_cpu.py builds it with the address and
// undefined-behaviour sanitizers): one env's world from a file, then a scripted walk — a pose, the carried slot, a clear flag and a
// mask byte per step —, each step one mwseen::update_one on the same map (a step under a zero mask byte is skipped, as the kernel
// skips the env).
//
// The file, whitespace-separated (doubles as Python's repr, which round-trips; nan is read as a NaN):
//   cell gx gz
//   range cos_half flags
//   fill count new             (what the map, its count and its new hold before the first step)
//   agent_radius max_forward_step
//   min_x max_x min_z max_z
//   nsegs, then ax az bx bz per segment
//   E, then kind x y z radius per slot
//   nsteps, then x z dir carry clear mask per step
// The answer, per step: "covered new count", then the gz * gx cells.
// `seen_map --policy N max_segs max_ents` prints mwpolicy::seen_launch instead: "grid threads lds fits".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../miniworld_amd/csrc/mw_policy.h"
#include "../../miniworld_amd/csrc/mw_seen.h"

static double rd(FILE *f)
{
    double v;
    if (fscanf(f, "%lf", &v) != 1) { fprintf(stderr, "seen_map: short file\n"); exit(2); }
    return v;
}
static int ri(FILE *f)
{
    int v;
    if (fscanf(f, "%d", &v) != 1) { fprintf(stderr, "seen_map: short file\n"); exit(2); }
    return v;
}

int main(int argc, char **argv)
{
    if (argc == 5 && !strcmp(argv[1], "--policy")) {
        const mwpolicy::SeenLaunch l = mwpolicy::seen_launch(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]));
        printf("%llu %d %zu %d\n", l.grid, l.threads, l.lds, l.fits ? 1 : 0);
        return 0;
    }
    if (argc != 2) { fprintf(stderr, "usage: seen_map WORLD | seen_map --policy N max_segs max_ents\n"); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    mw_nav_params p{};
    p.cell = rd(f); p.gx = ri(f); p.gz = ri(f);
    mwseen::Sight s{};
    s.range = rd(f); s.cos_half = rd(f); s.flags = ri(f);
    const int fill = ri(f);
    int32_t count = ri(f), newly = ri(f);
    MwRayArgs a{};
    a.w.agent_radius = rd(f); a.w.max_forward_step = rd(f);
    std::vector<double> extent(4);
    for (double &v : extent) v = rd(f);
    int32_t nsegs = ri(f);
    std::vector<double> segs((size_t)nsegs * 4 + 1);
    for (int i = 0; i < nsegs * 4; ++i) segs[i] = rd(f);
    const int E = ri(f);
    std::vector<int32_t> kind((size_t)E + 1);
    std::vector<double> pos((size_t)E * 3 + 1), geom((size_t)E * 9 + 1);
    for (int k = 0; k < E; ++k) {       // (the engine's layouts with N = 1: [3][E], [9][E])
        kind[k] = ri(f);
        for (int c = 0; c < 3; ++c) pos[(size_t)c * E + k] = rd(f);
        geom[(size_t)7 * E + k] = rd(f);
    }
    if (!(p.cell > 0.0) || p.gx < 1 || p.gz < 1 || (long long)p.gx * p.gz > MW_NAV_MAX_CELLS || !(s.range > 0.0) || !(s.cos_half >= -1.0 && s.cos_half <= 1.0) ||
        (s.flags & ~MW_SEEN_ENTITIES)) {
        fprintf(stderr, "seen_map: parameters the engine refuses\n");
        return 2;
    }
    uint32_t status = 0;
    int32_t carry = -1;
    double ax = 0.0, az = 0.0, adir = 0.0;
    a.w.segs = segs.data(); a.w.nsegs = &nsegs; a.w.extent = extent.data(); a.w.ekind = kind.data(); a.w.epos = pos.data(); a.w.egeom = geom.data();
    a.w.carry = &carry; a.w.ax = &ax; a.w.az = &az; a.w.status = &status;
    a.w.N = 1; a.w.E = E; a.w.max_segs = nsegs; a.w.shared_geom = 1;
    a.adir = &adir;
    const size_t cells = (size_t)p.gx * p.gz;
    std::vector<uint8_t> row(cells, (uint8_t)fill);
    std::vector<mwray::Wall> walls((size_t)nsegs + 1);
    std::vector<mwray::Disc> discs((size_t)E + 1);
    const int nsteps = ri(f);
    for (int t = 0; t < nsteps; ++t) {
        ax = rd(f); az = rd(f); adir = rd(f);
        carry = ri(f);
        const bool clear = ri(f) != 0, mask = ri(f) != 0;
        bool ok = true;
        if (mask) ok = mwseen::update_one(a, p, s, 0, clear, walls.data(), discs.data(), row.data(), &count, &newly);
        printf("%d %d %d\n", ok ? 1 : 0, (int)newly, (int)count);
        for (size_t c = 0; c < cells; ++c) printf("%u%c", (unsigned)row[c], c + 1 == cells ? '\n' : ' ');
    }
    fclose(f);
    return 0;
}
