// The host path of miniworld_amd/csrc/mw_ego.h, as a program of its own (tests/test_ego_cpu.py builds it with the address and
// undefined-behaviour sanitizers): one env's world and one source grid from a file, then a scripted walk — a pose, the carried slot, a
// mask byte and an optional origin per step —, each step one mwego::window_one into the same buffers (a step under a zero mask byte
// is skipped, as the kernel skips the env).
//
// The file (hostcheck.h: the tokens, the world block):
//   size cell back wall_radius entity_pad planes flags
//   range cos_half
//   src_bytes src_cell gx gz fill, then — src_bytes != 0 — the gz * gx elements of the source
//   garbage                    (the byte the planes and the sample hold before the first step)
//   the world: AGENT, EXTENT, SEGS, SLOTS
//   nsteps, then x z dir carry mask has_pos pos_x pos_z per step
// The answer, per step: a line with the P * size * size bytes of the planes ("-" without planes), a line with the size * size
// elements of the sample ("-" without a source).
// `ego_map --policy N max_segs max_ents planes` prints mwpolicy::ego_launch instead: "grid threads lds fits".
#define HOSTCHECK_PROGRAM "ego_map"
#include "hostcheck.h"

#include "../../miniworld_amd/csrc/mw_ego.h"
#include "../../miniworld_amd/csrc/mw_policy.h"

using namespace hostcheck;

int main(int argc, char **argv)
{
    if (argc == 6 && !strcmp(argv[1], "--policy")) {
        print_launch(mwpolicy::ego_launch(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5])));
        return 0;
    }
    if (argc != 2) { fprintf(stderr, "usage: ego_map WORLD | ego_map --policy N max_segs max_ents planes\n"); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    mwego::Window w{};
    w.size = ri(f); w.cell = rd(f); w.back = rd(f); w.wall_radius = rd(f); w.entity_pad = rd(f); w.planes = ri(f); w.flags = ri(f);
    const double range = rd(f), cos_half = rd(f);
    const mwseen::Sight s = mwego::sight_of(w, range, cos_half);
    mwego::Source q{};
    q.bytes = ri(f); q.cell = rd(f); q.gx = ri(f); q.gz = ri(f); q.fill = (uint32_t)ri(f);
    const bool sampled = q.bytes != 0;
    if (w.size < 1 || w.size > MW_EGO_MAX_SIZE || !(w.cell > 0.0) || !(w.wall_radius >= 0.0) || !(w.entity_pad >= 0.0) ||
        (w.planes & ~(MW_EGO_WALL | MW_EGO_ENTITY | MW_EGO_VISIBLE)) || (w.flags & ~(MW_EGO_ENTITIES | MW_EGO_NORTH)) || (!w.planes && !sampled) ||
        ((w.planes & MW_EGO_VISIBLE) && (!(range > 0.0) || !(cos_half >= -1.0 && cos_half <= 1.0))) ||
        (sampled && ((q.bytes != 1 && q.bytes != 2) || !(q.cell > 0.0) || q.gx < 1 || q.gz < 1 || (long long)q.gx * q.gz > MW_NAV_MAX_CELLS)))
        return refused();
    const size_t src_cells = sampled ? (size_t)q.gx * q.gz : 0;
    std::vector<uint8_t> src8(q.bytes == 1 ? src_cells : 0);
    std::vector<uint16_t> src16(q.bytes == 2 ? src_cells : 0);
    for (size_t c = 0; c < src_cells; ++c) {
        const int v = ri(f);
        if (q.bytes == 1) src8[c] = (uint8_t)v;
        else src16[c] = (uint16_t)v;
    }
    const int garbage = ri(f);
    World world;
    if (!world.read(f, AGENT | EXTENT | SEGS | SLOTS, (w.planes & MW_EGO_ENTITY) ? 255 : 1 << 20)) return refused();
    const MwRayArgs a = world.ray();
    const int P = mwego::plane_count(w.planes);
    const size_t cells = (size_t)w.size * w.size;
    // exactly as many bytes as the call may touch: the sanitizer sees a step past any of them
    std::vector<uint8_t> planes(P * cells, (uint8_t)garbage);
    std::vector<uint8_t> out8(q.bytes == 1 ? cells : 0, (uint8_t)garbage);
    std::vector<uint16_t> out16(q.bytes == 2 ? cells : 0, (uint16_t)(garbage * 0x101));
    std::vector<double> scratch((mwego::staged_bytes(world.nsegs, world.E, w.planes) + sizeof(double) - 1) / sizeof(double));
    const int nsteps = ri(f);
    for (int t = 0; t < nsteps; ++t) {
        world.ax = rd(f); world.az = rd(f); world.adir = rd(f);
        world.carry = ri(f);
        const bool mask = ri(f) != 0, has_pos = ri(f) != 0;
        const double origin[3] = {rd(f), 0.0, rd(f)};
        const void *src_row = q.bytes == 1 ? (const void *)src8.data() : q.bytes == 2 ? (const void *)src16.data() : nullptr;
        void *out_row = q.bytes == 1 ? (void *)out8.data() : q.bytes == 2 ? (void *)out16.data() : nullptr;
        if (mask) mwego::window_one(a, w, s, q, 0, has_pos ? origin : nullptr, scratch.data(), P ? planes.data() : nullptr, src_row, out_row);
        if (!P) printf("-");
        for (size_t c = 0; c < P * cells; ++c) printf("%u%s", (unsigned)planes[c], c + 1 == P * cells ? "" : " ");
        printf("\n");
        if (!sampled) printf("-");
        for (size_t c = 0; sampled && c < cells; ++c) printf("%u%s", q.bytes == 1 ? (unsigned)out8[c] : (unsigned)out16[c], c + 1 == cells ? "" : " ");
        printf("\n");
    }
    fclose(f);
    return 0;
}
