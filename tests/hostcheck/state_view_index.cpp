// The state views' index arithmetic (miniworld_amd/csrc/mw_state_view.h) on the host, as a program of its own so that it can run under
// the address and undefined-behaviour sanitizers (tests/test_state_view_cpu.py builds and runs it): for N = 5 envs of E = 3 slots,
// engine-side arrays filled with distinct values are gathered into rows and compared with the plain transposition mw_get_state
// performs (mw_engine.hip: state_xfer); rows are scattered back under the mask 1 0 1 0 1 and the unmasked columns must stay.
// Every array is a heap block of exactly its size: an index off by one is an error of the sanitizer, not a lucky read.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../miniworld_amd/csrc/mw_state_view.h"

namespace {

constexpr int N = 5, E = 3;
int failures = 0;

#define CHECK(cond, ...) do { if (!(cond)) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); ++failures; } } while (0)

// one field: its engine-side array(s) and the caller's rows
template <typename T>
struct Field {
    const char *name;
    int inner, slots;
    std::vector<T> dev, rows;
    Field(const char *n, int inner_, int slots_, int base) : name(n), inner(inner_), slots(slots_), dev((size_t)inner_ * slots_ * N), rows((size_t)N * slots_ * inner_)
    {
        for (size_t i = 0; i < dev.size(); ++i) dev[i] = (T)(base + (int)i);
    }
    // state_xfer's transposition: host [i][s][k] = component k of slot s, an array over the envs at (k * slots + s) * N
    T want(int i, int s, int k) const { return dev[((size_t)k * slots + s) * N + i]; }
};

struct World {
    Field<double> pos{"agent_pos", 3, 1, 1000}, dir{"agent_dir", 1, 1, 2000}, cam{"cam", 4, 1, 3000}, light{"light", 12, 1, 4000};
    Field<int32_t> carry{"carrying", 1, 1, 5000}, step{"step_count", 1, 1, 6000}, picked{"num_picked_up", 1, 1, 7000};
    Field<int32_t> ekind{"ent_kind", 1, E, 8000}, emesh{"ent_mesh", 1, E, 9000}, estatic{"ent_static", 1, E, 10000};
    Field<double> epos{"ent_pos", 3, E, 11000}, edir{"ent_dir", 1, E, 12000}, egeom{"ent_geom", 9, E, 13000}, extent{"extent", 4, 1, 14000};
    // agent_pos is three separate arrays in the engine: its [3][N] block is ax, ay, az in a row
    MwStateArrays arrays()
    {
        MwStateArrays a{};
        a.ax = pos.dev.data(); a.ay = pos.dev.data() + N; a.az = pos.dev.data() + 2 * N; a.adir = dir.dev.data(); a.cam = cam.dev.data(); a.light = light.dev.data();
        a.carry = carry.dev.data(); a.step = step.dev.data(); a.picked = picked.dev.data();
        a.ekind = ekind.dev.data(); a.emesh = emesh.dev.data(); a.estatic = estatic.dev.data();
        a.epos = epos.dev.data(); a.edir = edir.dev.data(); a.egeom = egeom.dev.data(); a.extent = extent.dev.data();
        return a;
    }
    mw_state_view view()
    {
        mw_state_view v{};
        v.agent_pos = pos.rows.data(); v.agent_dir = dir.rows.data(); v.cam = cam.rows.data(); v.light = light.rows.data();
        v.carrying = carry.rows.data(); v.step_count = step.rows.data(); v.num_picked_up = picked.rows.data();
        v.ent_kind = ekind.rows.data(); v.ent_mesh = emesh.rows.data(); v.ent_static = estatic.rows.data();
        v.ent_pos = epos.rows.data(); v.ent_dir = edir.rows.data(); v.ent_geom = egeom.rows.data(); v.extent = extent.rows.data();
        return v;
    }
    template <typename F>
    void each(F f) { f(pos); f(dir); f(cam); f(light); f(carry); f(step); f(picked); f(ekind); f(emesh); f(estatic); f(epos); f(edir); f(egeom); f(extent); }
};

}  // namespace

int main()
{
    // 1. gather: every field of every env, with one worker and with 64 (a wavefront's lanes, one after the other)
    for (int stride : {1, 64}) {
        World w;
        const MwStateArrays a = w.arrays();
        const mw_state_view v = w.view();
        for (int env = 0; env < N; ++env)
            for (int lane = 0; lane < stride; ++lane) mwsv::gather_env(a, v, E, N, (size_t)env, (size_t)env, lane, stride);
        w.each([&](auto &f) {
            for (int i = 0; i < N; ++i)
                for (int s = 0; s < f.slots; ++s)
                    for (int k = 0; k < f.inner; ++k)
                        CHECK(f.rows[((size_t)i * f.slots + s) * f.inner + k] == f.want(i, s, k), "gather %s env %d slot %d component %d (stride %d)", f.name, i, s, k, stride);
        });
    }
    // 2. a sub-range: envs 1 .. 3 into rows 0 .. 2 of buffers of exactly three rows
    {
        World w;
        const MwStateArrays a = w.arrays();
        w.each([](auto &f) { f.rows.resize((size_t)3 * f.slots * f.inner); f.rows.shrink_to_fit(); });
        const mw_state_view v = w.view();
        for (int item = 0; item < 3; ++item) mwsv::gather_env(a, v, E, N, (size_t)(1 + item), (size_t)item, 0, 1);
        w.each([&](auto &f) {
            for (int i = 0; i < 3; ++i)
                for (int s = 0; s < f.slots; ++s)
                    for (int k = 0; k < f.inner; ++k)
                        CHECK(f.rows[((size_t)i * f.slots + s) * f.inner + k] == f.want(1 + i, s, k), "range %s row %d slot %d component %d", f.name, i, s, k);
        });
    }
    // 3. scatter under the mask 1 0 1 0 1: masked columns take the rows, the others keep what they held
    {
        World w, src;
        const int mask[N] = {1, 0, 1, 0, 1};
        src.each([](auto &f) { for (size_t i = 0; i < f.rows.size(); ++i) f.rows[i] = (decltype(f.rows[0] + 0))(-1 - (int)i - 100 * f.inner); });
        World before = w;
        const MwStateArrays a = w.arrays();
        const mw_state_view v = src.view();
        for (int env = 0; env < N; ++env)
            if (mask[env])
                for (int lane = 0; lane < 64; ++lane) mwsv::scatter_env(a, v, E, N, (size_t)env, (size_t)env, lane, 64);
        // (pairs of fields in the same order)
        auto cmp = [&](auto &now, auto &old, auto &rows) {
            for (int i = 0; i < N; ++i)
                for (int s = 0; s < now.slots; ++s)
                    for (int k = 0; k < now.inner; ++k) {
                        const auto got = now.want(i, s, k);
                        const auto want = mask[i] ? rows.rows[((size_t)i * now.slots + s) * now.inner + k] : old.want(i, s, k);
                        CHECK(got == want, "scatter %s env %d slot %d component %d", now.name, i, s, k);
                    }
        };
        cmp(w.pos, before.pos, src.pos); cmp(w.dir, before.dir, src.dir); cmp(w.cam, before.cam, src.cam); cmp(w.light, before.light, src.light);
        cmp(w.carry, before.carry, src.carry); cmp(w.step, before.step, src.step); cmp(w.picked, before.picked, src.picked);
        cmp(w.ekind, before.ekind, src.ekind); cmp(w.emesh, before.emesh, src.emesh); cmp(w.estatic, before.estatic, src.estatic);
        cmp(w.epos, before.epos, src.epos); cmp(w.edir, before.edir, src.edir); cmp(w.egeom, before.egeom, src.egeom); cmp(w.extent, before.extent, src.extent);
    }
    // 4. a view with one field touches no other buffer (null pointers are never dereferenced), and the small predicates
    {
        World w;
        const MwStateArrays a = w.arrays();
        mw_state_view v{};
        CHECK(!mwsv::any_field(v), "an empty view names a field");
        v.agent_dir = w.dir.rows.data();
        CHECK(mwsv::any_field(v), "a view with agent_dir names none");
        for (int env = 0; env < N; ++env) mwsv::gather_env(a, v, E, N, (size_t)env, (size_t)env, 0, 1);
        for (int i = 0; i < N; ++i) CHECK(w.dir.rows[i] == w.dir.want(i, 0, 0), "agent_dir alone, env %d", i);
        for (double x : w.epos.rows) CHECK(x == 0.0, "a buffer that was not named was written");
        CHECK(mwsv::carrying_ok(-1, E) && mwsv::carrying_ok(E - 1, E) && !mwsv::carrying_ok(E, E) && !mwsv::carrying_ok(-2, E), "carrying_ok");
        CHECK(mwsv::kind_ok(MW_ENT_NONE) && mwsv::kind_ok(MW_ENT_FRAME) && !mwsv::kind_ok(MW_ENT_FRAME + 1) && !mwsv::kind_ok(-1) && !mwsv::kind_ok(9), "kind_ok");
        CHECK(mwsv::row_index<9>(2, 4) == 22 && mwsv::dev_index<9>(22, E, N, 3) == ((size_t)4 * E + 2) * N + 3, "row_index / dev_index");
    }
    std::printf(failures ? "state_view_index: %d failures\n" : "state_view_index: ok\n", failures);
    return failures ? 1 : 0;
}
