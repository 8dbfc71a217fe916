// The host path of miniworld_amd/csrc/mw_ray.h, as a program of its own (tests/test_ray_cpu.py builds it with the address and
// undefined-behaviour sanitizers): one env's world from a file, a fan of rays from the agent and explicit rays, each through
// mwray::ray_of and mwray::cast_one.
//
// The file, whitespace-separated (doubles as Python's repr, which round-trips; nan is read as a NaN):
//   max_t radius flags
//   agent_radius max_forward_step carry
//   agent_x agent_z agent_dir
//   nsegs, then ax az bx bz per segment
//   E, then kind x y z radius per slot
//   nfan, then the offsets
//   nrays, then ox oy oz dx dz per explicit ray
// The answer: "t hit dx dz" per ray (%a, %d), the fan first.
// `ray_cast --policy N R max_segs max_ents` prints mwpolicy::ray_launch instead: "per_lane grid threads lds fits threshold".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../miniworld_amd/csrc/mw_policy.h"
#include "../../miniworld_amd/csrc/mw_ray.h"

static double rd(FILE *f)
{
    double v;
    if (fscanf(f, "%lf", &v) != 1) { fprintf(stderr, "ray_cast: short file\n"); exit(2); }
    return v;
}
static int ri(FILE *f)
{
    int v;
    if (fscanf(f, "%d", &v) != 1) { fprintf(stderr, "ray_cast: short file\n"); exit(2); }
    return v;
}

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
    MwRayArgs a{};
    a.w.agent_radius = rd(f); a.w.max_forward_step = rd(f);
    int32_t carry = ri(f);
    double ax = rd(f), az = rd(f), adir = rd(f);
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
    const int nfan = ri(f);
    std::vector<double> offsets((size_t)nfan + 1);
    for (int i = 0; i < nfan; ++i) offsets[i] = rd(f);
    const int nrays = ri(f);
    std::vector<double> origin((size_t)nrays * 3 + 1), dir((size_t)nrays * 2 + 1);
    for (int i = 0; i < nrays; ++i) {
        for (int k = 0; k < 3; ++k) origin[(size_t)i * 3 + k] = rd(f);
        for (int k = 0; k < 2; ++k) dir[(size_t)i * 2 + k] = rd(f);
    }
    fclose(f);
    if (nfan > MW_RAY_MAX || nrays > MW_RAY_MAX || !(p.max_t > 0.0) || !(p.radius >= 0.0) || (p.flags & ~MW_RAY_ENTITIES)) {
        fprintf(stderr, "ray_cast: parameters the engine refuses\n");
        return 2;
    }
    uint32_t status = 0;
    a.w.segs = segs.data(); a.w.nsegs = &nsegs; a.w.extent = nullptr; a.w.ekind = kind.data(); a.w.epos = pos.data(); a.w.egeom = geom.data();
    a.w.carry = &carry; a.w.ax = &ax; a.w.az = &az; a.w.status = &status;
    a.w.N = 1; a.w.E = E; a.w.max_segs = nsegs; a.w.shared_geom = 1;
    a.adir = &adir;
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
