// The host path of miniworld_amd/csrc/mw_depth.h, as a program of its own (tests/test_depth_cpu.py builds it with the address and
// undefined-behaviour sanitizers): one env's extent and one target from a file, then a scripted walk — a pose, a camera, a mask byte, a
// clear byte and a depth map per step —, each step one mwdepth::window_one or map_one into the same buffers (a step under a zero mask
// byte is skipped, as the kernel skips the env).
//
// The file (hostcheck.h: the tokens, the world block; depth values as the hexadecimal bits of their float32):
//   W H msaa
//   min_range max_range floor_tol top
//   target                     0: then size cell back flags;  1: then cell gx gz min_points
//   garbage                    (the byte the planes, the map and the counts' bytes hold before the first step)
//   the world: EXTENT alone (the projection reads neither segments nor slots)
//   nsteps, then per step: x z dir  cam_height cam_fwd_disp cam_pitch cam_fov_y  mask clear, then H * W depth words
// The answer, per step: a line with the 2 * cells bytes of the planes or the map; for a map a second line "count0 count1 new0 new1".
// `depth_project --policy N cells` prints mwpolicy::depth_launch instead: "grid threads lds fits"; `depth_project --pattern msaa` prints
// mwdepth::sample0_of: "sx sy".
#define HOSTCHECK_PROGRAM "depth_project"
#include "hostcheck.h"

#include "../../miniworld_amd/csrc/mw_depth.h"
#include "../../miniworld_amd/csrc/mw_policy.h"

using namespace hostcheck;

int main(int argc, char **argv)
{
    if (argc == 4 && !strcmp(argv[1], "--policy")) {
        print_launch(mwpolicy::depth_launch(atoi(argv[2]), atoll(argv[3])));
        return 0;
    }
    if (argc == 3 && !strcmp(argv[1], "--pattern")) {
        int sx, sy;
        mwdepth::sample0_of(atoi(argv[2]), sx, sy);
        printf("%d %d\n", sx, sy);
        return 0;
    }
    if (argc != 2) { fprintf(stderr, "usage: depth_project WALK | depth_project --policy N cells | depth_project --pattern msaa\n"); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    mwdepth::Sensor s{};
    s.W = ri(f); s.H = ri(f);
    const int msaa = ri(f);
    s.min_range = rd(f); s.max_range = rd(f); s.floor_tol = rd(f); s.top = rd(f);
    mwdepth::subpixel_of(msaa, s.sub_x, s.sub_y);
    const bool to_map = ri(f) != 0;
    mwdepth::Window w{1.0, 0.0, 1, 0};
    mw_nav_params p{1.0, 0.0, 0.0, 1, 1, 0, 0};
    int min_points = 1;
    if (to_map) {
        p.cell = rd(f); p.gx = ri(f); p.gz = ri(f); min_points = ri(f);
    } else {
        w.size = ri(f); w.cell = rd(f); w.back = rd(f); w.flags = ri(f);
    }
    const long long cells = to_map ? (long long)p.gx * p.gz : (long long)w.size * w.size;
    if (s.W < 1 || s.H < 1 || (long long)s.W * s.H > MW_DEPTH_MAX_PIXELS || !(s.min_range > 0.0) || !(s.max_range >= s.min_range) || !(s.floor_tol >= 0.0) ||
        !(s.top >= s.floor_tol) || (msaa != 1 && msaa != 4 && msaa != 8) ||
        (to_map ? (!(p.cell > 0.0) || p.gx < 1 || p.gz < 1 || min_points < 1 || min_points > 255)
                : (w.size < 1 || w.size > MW_EGO_MAX_SIZE || !(w.cell > 0.0) || (w.flags & ~MW_EGO_NORTH))) ||
        !mwpolicy::depth_launch(1, cells).fits)
        return refused();
    const int garbage = ri(f);
    World world;
    world.read(f, EXTENT);
    const MwRayArgs a = world.ray();
    double cam[4] = {0.0, 0.0, 0.0, 0.0};
    // exactly as many elements as the call may touch: the sanitizer sees a step past any of them
    std::vector<uint8_t> out(2 * (size_t)cells, (uint8_t)garbage);
    std::vector<uint32_t> scratch((size_t)cells);
    std::vector<float> depth((size_t)s.W * s.H);
    int32_t count[2], newly[2];
    memset(count, garbage, sizeof count);
    memset(newly, garbage, sizeof newly);
    const int nsteps = ri(f);
    for (int t = 0; t < nsteps; ++t) {
        world.ax = rd(f); world.az = rd(f); world.adir = rd(f);
        for (double &v : cam) v = rd(f);
        const bool mask = ri(f) != 0, clear = ri(f) != 0;
        for (float &v : depth) v = rbits(f);
        if (mask) {
            if (to_map) mwdepth::map_one(a, cam, s, p, min_points, 0, clear, depth.data(), scratch.data(), out.data(), count, newly);
            else mwdepth::window_one(a, cam, s, w, 0, depth.data(), scratch.data(), out.data());
        }
        for (size_t c = 0; c < out.size(); ++c) printf("%u%s", (unsigned)out[c], c + 1 == out.size() ? "" : " ");
        printf("\n");
        if (to_map) printf("%d %d %d %d\n", (int)count[0], (int)count[1], (int)newly[0], (int)newly[1]);
    }
    fclose(f);
    return 0;
}
