// The host path of miniworld_amd/csrc/mw_clear.h, as a program of its own (tests/test_clearance_cpu.py builds it with the address and
// undefined-behaviour sanitizers): one env's marked grid from a file and, for each of the file's calls, mwclear::clear_one's outputs.
//
// The file (hostcheck.h: the tokens):  gx gz shift calls;  gz * gx bytes of marked;  per call: limit want_nearest B, then B pairs thr cost.
// `shift` (0 .. 3) is the marked row's distance from a 4-byte boundary; every array holds exactly the elements a call may touch.
// The answer, per call: the dist2, with want_nearest the nearest, with B > 0 the costs, a row of gz * gx each.
// `grid_clearance --policy N cells` prints mwpolicy::clear_launch: "grid threads lds fits".
#define HOSTCHECK_PROGRAM "grid_clearance"
#include "hostcheck.h"

#include "../../miniworld_amd/csrc/mw_clear.h"
#include "../../miniworld_amd/csrc/mw_policy.h"

using namespace hostcheck;

int main(int argc, char **argv)
{
    const auto print_row = [](const auto &v) { for (size_t c = 0; c < v.size(); ++c) printf("%d%c", (int)v[c], c + 1 == v.size() ? '\n' : ' '); };
    if (argc == 4 && !strcmp(argv[1], "--policy")) {
        print_launch(mwpolicy::clear_launch(atoi(argv[2]), atoll(argv[3])));
        return 0;
    }
    FILE *f = argc == 2 ? fopen(argv[1], "r") : nullptr;
    if (!f) return 2;
    const int gx = ri(f), gz = ri(f), shift = ri(f), calls = ri(f);
    const size_t cells = (size_t)gx * gz;
    std::vector<uint8_t> store(cells + (size_t)shift);
    uint8_t *marked = store.data() + shift;
    for (size_t c = 0; c < cells; ++c) marked[c] = (uint8_t)ri(f);
    for (int call = 0; call < calls; ++call) {
        const int limit = ri(f);
        const bool want_nearest = ri(f) != 0;
        const int B = ri(f);
        std::vector<int32_t> pairs((size_t)B * 2);
        for (int32_t &v : pairs) v = ri(f);
        if (mwclear::bands_error(pairs.data(), B)) return refused();
        std::vector<int16_t> off(cells);
        std::vector<int32_t> dist2(cells, -7), nearest(want_nearest ? cells : 0, -7);
        std::vector<uint8_t> cost(B ? cells : 0, 7);
        mwclear::clear_one(gx, gz, limit, mwclear::make_bands(pairs.data(), B), marked, off.data(), dist2.data(), want_nearest ? nearest.data() : nullptr,
                           B ? cost.data() : nullptr);
        print_row(dist2);
        if (want_nearest) print_row(nearest);
        if (B) print_row(cost);
    }
    fclose(f);
    return 0;
}
