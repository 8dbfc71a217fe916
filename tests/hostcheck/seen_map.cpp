// The host path of miniworld_amd/csrc/mw_seen.h, as a program of its own (tests/test_seen_cpu.py builds it with the address and
// undefined-behaviour sanitizers): one env's world from a file, then a scripted walk — a pose, the carried slot, a clear flag and a
// mask byte per step —, each step one mwseen::update_one on the same map (a step under a zero mask byte is skipped, as the kernel
// skips the env).
//
// The file (hostcheck.h: the tokens, the world block):
//   cell gx gz
//   range cos_half flags
//   fill count new             (what the map, its count and its new hold before the first step)
//   the world: AGENT, EXTENT, SEGS, SLOTS
//   nsteps, then x z dir carry clear mask per step
// The answer, per step: "covered new count", then the gz * gx cells.
// `seen_map --policy N max_segs max_ents` prints mwpolicy::seen_launch instead: "grid threads lds fits".
#define HOSTCHECK_PROGRAM "seen_map"
#include "hostcheck.h"

#include "../../miniworld_amd/csrc/mw_policy.h"
#include "../../miniworld_amd/csrc/mw_seen.h"

using namespace hostcheck;

int main(int argc, char **argv)
{
    if (argc == 5 && !strcmp(argv[1], "--policy")) {
        print_launch(mwpolicy::seen_launch(atoi(argv[2]), atoi(argv[3]), atoi(argv[4])));
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
    World world;
    if (!world.read(f, AGENT | EXTENT | SEGS | SLOTS)) return refused();
    if (!(p.cell > 0.0) || p.gx < 1 || p.gz < 1 || (long long)p.gx * p.gz > MW_NAV_MAX_CELLS || !(s.range > 0.0) || !(s.cos_half >= -1.0 && s.cos_half <= 1.0) ||
        (s.flags & ~MW_SEEN_ENTITIES))
        return refused();
    const MwRayArgs a = world.ray();
    const size_t cells = (size_t)p.gx * p.gz;
    std::vector<uint8_t> row(cells, (uint8_t)fill);
    std::vector<mwray::Wall> walls((size_t)world.nsegs);
    std::vector<mwray::Disc> discs((size_t)world.E);
    const int nsteps = ri(f);
    for (int t = 0; t < nsteps; ++t) {
        world.ax = rd(f); world.az = rd(f); world.adir = rd(f);
        world.carry = ri(f);
        const bool clear = ri(f) != 0, mask = ri(f) != 0;
        bool ok = true;
        if (mask) ok = mwseen::update_one(a, p, s, 0, clear, walls.data(), discs.data(), row.data(), &count, &newly);
        printf("%d %d %d\n", ok ? 1 : 0, (int)newly, (int)count);
        for (size_t c = 0; c < cells; ++c) printf("%u%c", (unsigned)row[c], c + 1 == cells ? '\n' : ' ');
    }
    fclose(f);
    return 0;
}
