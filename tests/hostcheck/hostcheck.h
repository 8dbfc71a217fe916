// What the world-query programs beside this file share (nav_field, ray_cast, seen_map, ego_map, depth_project, label_frame; each is
// built with the address and undefined-behaviour sanitizers by its tests/test_*_cpu.py): the token readers, the "refused" exit, one
// env's world in the engine's layouts, and the printer of a launch.  A program names itself before the include:
//     #define HOSTCHECK_PROGRAM "nav_field"
//
// Every file is whitespace-separated tokens: doubles as Python's repr, which round-trips (nan is read as a NaN), float32 values as the
// hexadecimal bits of their float32, so that a NaN, an infinity and a negative zero arrive as they are.
//
// The world block of a file, of which a program reads the parts it names (World::read) in this order:
//   AGENT    agent_radius max_forward_step, and with CARRY the carried slot behind them
//   POSE     agent_x agent_z agent_dir
//   EXTENT   min_x max_x min_z max_z
//   SEGS     nsegs, then ax az bx bz per segment
//   SLOTS    E, then kind x y z radius per slot; with WIDE instead kind mesh  pos[3] dir geom[9]
#pragma once
#ifndef HOSTCHECK_PROGRAM
#error "define HOSTCHECK_PROGRAM, the program's name in its messages, before hostcheck.h"
#endif
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../miniworld_amd/csrc/mw_ray.h"

namespace hostcheck {

[[noreturn]] static void short_file()
{
    fprintf(stderr, HOSTCHECK_PROGRAM ": short file\n");
    exit(2);
}
static double rd(FILE *f)
{
    double v;
    if (fscanf(f, "%lf", &v) != 1) short_file();
    return v;
}
static int ri(FILE *f)
{
    int v;
    if (fscanf(f, "%d", &v) != 1) short_file();
    return v;
}
[[maybe_unused]] static float rbits(FILE *f)
{
    unsigned v;
    if (fscanf(f, "%x", &v) != 1) short_file();
    const uint32_t u = v;
    float x;
    memcpy(&x, &u, 4);
    return x;
}

// main's `return refused();` for a file whose parameters the engine's entry point would refuse
static int refused()
{
    fprintf(stderr, HOSTCHECK_PROGRAM ": parameters the engine refuses\n");
    return 2;
}

// "grid threads lds fits" of a mwpolicy launch (`--policy`)
template <typename L>
static void print_launch(const L &l)
{
    printf("%llu %d %zu %d\n", l.grid, l.threads, l.lds, l.fits ? 1 : 0);
}

enum : unsigned { AGENT = 1, CARRY = 2, POSE = 4, EXTENT = 8, SEGS = 16, SLOTS = 32, WIDE = 64 };

// One env's world, in the engine's layouts with N = 1 and shared geometry: [E], [3][E], [9][E].  Every array holds exactly as many
// elements as a call may touch — the sanitizer sees a step past any of them —, and a part the program did not read is a null pointer.
// The views point into the World: it stays where it is while they are in use.
struct World {
    double agent_radius = 0.0, max_forward_step = 0.0, ax = 0.0, az = 0.0, adir = 0.0;
    int32_t carry = -1, nsegs = 0;
    int E = 0;
    uint32_t status = 0;
    std::vector<double> extent, segs, epos, edir, egeom;
    std::vector<int32_t> ekind, emesh;

    World() = default;
    World(const World &) = delete;
    World &operator=(const World &) = delete;

    // false for counts no array can be made of, or more than max_slots slots: the caller refuses
    bool read(FILE *f, unsigned parts, int max_slots = 1 << 20)
    {
        if (parts & AGENT) {
            agent_radius = rd(f); max_forward_step = rd(f);
            if (parts & CARRY) carry = ri(f);
        }
        if (parts & POSE) { ax = rd(f); az = rd(f); adir = rd(f); }
        if (parts & EXTENT) {
            extent.resize(4);
            for (double &v : extent) v = rd(f);
        }
        if (parts & SEGS) {
            nsegs = ri(f);
            if (nsegs < 0) return false;
            segs.resize((size_t)nsegs * 4);
            for (double &v : segs) v = rd(f);
        }
        if (parts & SLOTS) {
            E = ri(f);
            if (E < 0 || E > max_slots) return false;
            ekind.resize((size_t)E); epos.resize((size_t)E * 3); egeom.resize((size_t)E * 9);
            if (parts & WIDE) { emesh.resize((size_t)E); edir.resize((size_t)E); }
            for (int s = 0; s < E; ++s) {
                ekind[s] = ri(f);
                if (parts & WIDE) emesh[s] = ri(f);
                for (int k = 0; k < 3; ++k) epos[(size_t)k * E + s] = rd(f);
                if (parts & WIDE) {
                    edir[s] = rd(f);
                    for (int k = 0; k < 9; ++k) egeom[(size_t)k * E + s] = rd(f);
                } else {
                    egeom[(size_t)7 * E + s] = rd(f);      // (the radius; the rest of a slot's geometry stays 0)
                }
            }
        }
        return true;
    }

    // what the nav calls read: no agent pose
    MwNavArgs nav()
    {
        MwNavArgs a{};
        a.segs = segs.data(); a.nsegs = &nsegs; a.extent = extent.data(); a.ekind = ekind.data(); a.epos = epos.data(); a.egeom = egeom.data();
        a.carry = &carry; a.ax = nullptr; a.az = nullptr; a.status = &status;
        a.N = 1; a.E = E; a.max_segs = nsegs; a.shared_geom = 1;
        a.agent_radius = agent_radius; a.max_forward_step = max_forward_step;
        return a;
    }
    // ... and with the agent's pose, which a scripted walk writes into ax, az, adir (and carry) step by step
    MwRayArgs ray()
    {
        MwRayArgs a{};
        a.w = nav();
        a.w.ax = &ax; a.w.az = &az;
        a.adir = &adir;
        return a;
    }
};

}  // namespace hostcheck
