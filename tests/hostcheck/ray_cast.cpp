// The host path of miniworld_amd/csrc/mw_ray.h, as a program of its own (tests/test_ray_cpu.py builds it with the address and
// undefined-behaviour sanitizers): one env's world from a file, a fan of rays from the agent and explicit rays, each through
// mwray::ray_of and mwray::cast_one.
//
// The file (hostcheck.h: the tokens, the world block):
//   max_t radius flags
//   the world: AGENT with CARRY, POSE, SEGS, SLOTS (no extent: a cast reads none)
//   nfan, then the offsets
//   nrays, then ox oy oz dx dz per explicit ray
// The answer: "t hit dx dz" per ray (%a, %d), the fan first.
// `ray_cast --policy N R max_segs max_ents` prints mwpolicy::ray_launch instead: "per_lane grid threads lds fits threshold".
#define HOSTCHECK_PROGRAM "ray_cast"
#include "hostcheck.h"

#include "../../miniworld_amd/csrc/mw_policy.h"
#include "../../miniworld_amd/csrc/mw_ray.h"

using namespace hostcheck;

int main(int argc, char **argv)
{
    if (argc == 6 && !strcmp(argv[1], "--policy")) {
        const mwpolicy::RayLaunch l = mwpolicy::ray_launch(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]));
        printf("%d %llu %d %zu %d %d\n", l.per_lane ? 1 : 0, l.grid, l.threads, l.lds, l.fits ? 1 : 0, mwpolicy::kRayPerLaneFrom);
        return 0;
    }
    if (argc != 2) { fprintf(stderr, "usage: ray_cast WORLD | ray_cast --policy N R max_segs max_ents\n"); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    mw_ray_params p{};
    p.max_t = rd(f); p.radius = rd(f); p.flags = ri(f);
    World world;
    if (!world.read(f, AGENT | CARRY | POSE | SEGS | SLOTS)) return refused();
    const int nfan = ri(f);
    std::vector<double> offsets((size_t)(nfan > 0 ? nfan : 0));
    for (double &v : offsets) v = rd(f);
    const int nrays = ri(f);
    std::vector<double> origin((size_t)(nrays > 0 ? nrays : 0) * 3), dir((size_t)(nrays > 0 ? nrays : 0) * 2);
    for (int i = 0; i < nrays; ++i) {
        for (int k = 0; k < 3; ++k) origin[(size_t)i * 3 + k] = rd(f);
        for (int k = 0; k < 2; ++k) dir[(size_t)i * 2 + k] = rd(f);
    }
    fclose(f);
    if (nfan > MW_RAY_MAX || nrays > MW_RAY_MAX || !(p.max_t > 0.0) || !(p.radius >= 0.0) || (p.flags & ~MW_RAY_ENTITIES))
        return refused();
    const MwRayArgs a = world.ray();
    for (int pass = 0; pass < 2; ++pass) {
        p.rays = pass == 0 ? nfan : nrays;
        for (int k = 0; k < p.rays; ++k) {
            const mwray::Ray r = pass == 0 ? mwray::ray_of(a, p, 0, k, nullptr, nullptr, offsets.data())
                                           : mwray::ray_of(a, p, 0, k, origin.data(), dir.data(), nullptr);
            const mwray::Hit h = mwray::cast_one(a, p, 0, r);
            printf("%a %d %a %a\n", h.t, (int)h.code, r.dx, r.dz);
        }
    }
    return 0;
}
