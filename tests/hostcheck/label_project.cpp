// The host path of miniworld_amd/csrc/mw_labelmap.h, as a program of its own (tests/test_labelmap_cpu.py builds it with the address and
// undefined-behaviour sanitizers): one env's extent and one target from a file, then a scripted walk — a pose, a camera, a mask byte, a
// clear byte, a depth map and a label image per step —, each step one mwlabelmap::window_one or map_one into the same buffers (a step
// under a zero mask byte is skipped, as the kernel skips the env).
//
// The file (hostcheck.h: the tokens, the world block; depth values as the hexadecimal bits of their float32):
//   W H msaa
//   min_range max_range floor_tol top
//   base
//   target                     0: then size cell back flags;  1: then cell gx gz ids
//   garbage                    (the byte the plane, the map and the per-object outputs' bytes hold before the first step)
//   the world: EXTENT alone (the projection reads neither segments nor slots)
//   nsteps, then per step: x z dir  cam_height cam_fwd_disp cam_pitch cam_fov_y  mask clear, then H * W depth words, then H * W codes
// The answer, per step: a line with the cells' bytes of the plane or the map; for a map a second line with the ids' cell counts and a
// third with the 3 * ids positions as the hexadecimal bits of their float64 (both empty with ids = 0).
// `label_project --policy N cells ids` prints mwpolicy::labelmap_launch instead: "grid threads lds fits".
#define HOSTCHECK_PROGRAM "label_project"
#include "hostcheck.h"

#include "../../miniworld_amd/csrc/mw_labelmap.h"
#include "../../miniworld_amd/csrc/mw_policy.h"

using namespace hostcheck;

int main(int argc, char **argv)
{
    if (argc == 5 && !strcmp(argv[1], "--policy")) {
        print_launch(mwpolicy::labelmap_launch(atoi(argv[2]), atoll(argv[3]), atoi(argv[4])));
        return 0;
    }
    if (argc != 2) { fprintf(stderr, "usage: label_project WALK | label_project --policy N cells ids\n"); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    mwdepth::Sensor s{};
    s.W = ri(f); s.H = ri(f);
    const int msaa = ri(f);
    s.min_range = rd(f); s.max_range = rd(f); s.floor_tol = rd(f); s.top = rd(f);
    mwdepth::subpixel_of(msaa, s.sub_x, s.sub_y);
    const int32_t base = ri(f);
    const bool to_map = ri(f) != 0;
    mwdepth::Window w{1.0, 0.0, 1, 0};
    mw_nav_params p{1.0, 0.0, 0.0, 1, 1, 0, 0};
    int K = 0;
    if (to_map) {
        p.cell = rd(f); p.gx = ri(f); p.gz = ri(f); K = ri(f);
    } else {
        w.size = ri(f); w.cell = rd(f); w.back = rd(f); w.flags = ri(f);
    }
    const long long cells = to_map ? (long long)p.gx * p.gz : (long long)w.size * w.size;
    if (s.W < 1 || s.H < 1 || (long long)s.W * s.H > MW_DEPTH_MAX_PIXELS || !(s.min_range > 0.0) || !(s.max_range >= s.min_range) || !(s.floor_tol >= 0.0) ||
        !(s.top >= s.floor_tol) || (msaa != 1 && msaa != 4 && msaa != 8) || base < 0 ||
        (to_map ? (!(p.cell > 0.0) || p.gx < 1 || p.gz < 1) : (w.size < 1 || w.size > MW_EGO_MAX_SIZE || !(w.cell > 0.0) || (w.flags & ~MW_EGO_NORTH))) ||
        !mwpolicy::labelmap_launch(1, cells, K).fits)
        return refused();
    const int garbage = ri(f);
    World world;
    world.read(f, EXTENT);
    const MwRayArgs a = world.ray();
    double cam[4] = {0.0, 0.0, 0.0, 0.0};
    // exactly as many elements as the call may touch: the sanitizer sees a step past any of them
    std::vector<uint8_t> out((size_t)cells, (uint8_t)garbage);
    std::vector<uint32_t> keys((size_t)cells + 3 * (size_t)K);
    std::vector<float> depth((size_t)s.W * s.H);
    std::vector<int32_t> code((size_t)s.W * s.H);
    std::vector<int32_t> obj_cells((size_t)K);
    std::vector<double> obj_pos((size_t)K * 3);
    if (K) {
        memset(obj_cells.data(), garbage, obj_cells.size() * sizeof(int32_t));
        memset(obj_pos.data(), garbage, obj_pos.size() * sizeof(double));
    }
    // the engine's rule for the 16-byte loads, on the host's own addresses
    const bool wide = (s.W * s.H) % 4 == 0 && mwpolicy::wide_units((uintptr_t)depth.data() | (uintptr_t)code.data());
    const int nsteps = ri(f);
    for (int t = 0; t < nsteps; ++t) {
        world.ax = rd(f); world.az = rd(f); world.adir = rd(f);
        for (double &v : cam) v = rd(f);
        const bool mask = ri(f) != 0, clear = ri(f) != 0;
        for (float &v : depth) v = rbits(f);
        for (int32_t &v : code) v = ri(f);
        if (mask) {
            if (to_map)
                mwlabelmap::map_one(a, cam, s, p, 0, clear, depth.data(), code.data(), base, wide, keys.data(), out.data(), K, K ? obj_cells.data() : nullptr,
                                    K ? obj_pos.data() : nullptr);
            else mwlabelmap::window_one(a, cam, s, w, 0, depth.data(), code.data(), base, wide, keys.data(), out.data());
        }
        for (size_t c = 0; c < out.size(); ++c) printf("%u%s", (unsigned)out[c], c + 1 == out.size() ? "" : " ");
        printf("\n");
        if (to_map) {
            for (int q = 0; q < K; ++q) printf("%d%s", (int)obj_cells[q], q + 1 == K ? "" : " ");
            printf("\n");
            for (int q = 0; q < 3 * K; ++q) {
                uint64_t bits;
                memcpy(&bits, &obj_pos[(size_t)q], 8);
                printf("%llx%s", (unsigned long long)bits, q + 1 == 3 * K ? "" : " ");
            }
            printf("\n");
        }
    }
    fclose(f);
    return 0;
}
