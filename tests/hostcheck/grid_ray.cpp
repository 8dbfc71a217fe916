// The host path of miniworld_amd/csrc/mw_gridray.h, as a program of its own (tests/test_grid_ray_cpu.py builds it with the address and
// undefined-behaviour sanitizers): one env's rays by mwgray::cast_one, under either form's walk.
// The file (hostcheck.h: the tokens):  the world's EXTENT;  cell gx gz shift max_t R;  R rays: ox oz dx dz;  gz * gx opaque bytes.
// `shift` (0 .. 3) is the opaque row's distance from a 4-byte boundary; every array holds exactly the elements a call may touch.  The
// answer, per form — the staged walk over bits, the unstaged batches over bytes — a row per ray: the bits of t in hexadecimal, and hit.
// `grid_ray --policy N cells rays forced` prints mwpolicy::gridray_launch, with "staged" behind the four.
#define HOSTCHECK_PROGRAM "grid_ray"
#include "hostcheck.h"

#include "../../miniworld_amd/csrc/mw_gridray.h"
#include "../../miniworld_amd/csrc/mw_policy.h"

using namespace hostcheck;

int main(int argc, char **argv)
{
    if (argc == 6 && !strcmp(argv[1], "--policy")) {
        const mwpolicy::GridRayLaunch l = mwpolicy::gridray_launch(atoi(argv[2]), atoll(argv[3]), atoi(argv[4]), atoi(argv[5]));
        printf("%llu %d %zu %d %d\n", l.grid, l.threads, l.lds, l.fits ? 1 : 0, l.staged ? 1 : 0);
        return 0;
    }
    FILE *f = argc == 2 ? fopen(argv[1], "r") : nullptr;
    if (!f) return 2;
    World w;
    if (!w.read(f, EXTENT)) return refused();
    mw_nav_params p{};
    p.cell = rd(f); p.gx = ri(f); p.gz = ri(f);
    const int shift = ri(f); const double max_t = rd(f); const int R = ri(f);
    const size_t cells = (size_t)p.gx * p.gz;
    if (!mwpolicy::gridray_launch(1, (long long)cells, R).fits || !(max_t > 0.0)) return refused();
    std::vector<double> origin((size_t)R * 3, 0.0), dir((size_t)R * 2);
    for (int k = 0; k < R; ++k) { origin[3 * k] = rd(f); origin[3 * k + 2] = rd(f); dir[2 * k] = rd(f); dir[2 * k + 1] = rd(f); }
    std::vector<uint8_t> store(cells + (size_t)shift);
    for (size_t c = 0; c < cells; ++c) store[shift + c] = (uint8_t)ri(f);
    fclose(f);
    const uint8_t *opaque = store.data() + shift;
    const MwRayArgs a = w.ray();
    const mwnav::Grid g = mwnav::grid_of(a.w, p, 0);
    if (!mwnav::covers(g)) return refused();
    std::vector<uint32_t> bits((cells + 31) / 32);
    mwsight::zero_bits(bits.data(), (int)cells, 0, 1);
    mwsight::stage_bits(opaque, bits.data(), (int)cells, 0, 1, [](uint32_t *word, uint32_t bit) { *word |= bit; });
    for (int form = 0; form < 2; ++form)
        for (int k = 0; k < R; ++k) {
            const mwray::Ray r = mwray::ray_of(a, mwgray::fan_of(R, max_t), 0, k, origin.data(), dir.data(), nullptr);
            const mwray::Hit h = mwgray::cast_one(g, r, max_t, opaque, bits.data(), form);
            printf("%016llx %d\n", (unsigned long long)mwgray::to_bits(h.t), (int)h.code);
        }
    return 0;
}
