// The host path of miniworld_amd/csrc/mw_regions.h, as a program of its own (tests/test_regions_cpu.py builds it with the address and
// undefined-behaviour sanitizers): one env's member grid from a file and, for each of the file's calls, the outputs of
// mwregions::regions_one.
//
// The file (hostcheck.h: the tokens):
//   cell gx gz shift calls          (cell: the grid's, checked as the entry point checks it and not read otherwise)
//   gz * gx bytes of member
//   per call: connectivity min_cells K want_sum want_label
// `shift` (0 .. 3) is the distance of the member row from a 4-byte boundary, and the row is the last bytes of an allocation of its own, so
// that the sanitizer sees a read past either end (nav_grid.cpp's rows).  Every array of a call holds exactly the elements the call may
// touch: cells labels and sizes, K entries, K sizes and cells, 2 K sums, cells label codes.
// The answer, per call: "regions <count> <rounds>", the K sizes, the K cells, with want_sum the 2 K sums, with want_label the gz * gx
// codes.
//
// `grid_regions --policy N cells max_regions` prints mwpolicy::regions_launch: "grid threads lds fits".
#define HOSTCHECK_PROGRAM "grid_regions"
#include "hostcheck.h"

#include "../../miniworld_amd/csrc/mw_policy.h"
#include "../../miniworld_amd/csrc/mw_regions.h"

using namespace hostcheck;

int main(int argc, char **argv)
{
    if (argc == 5 && !strcmp(argv[1], "--policy")) {
        print_launch(mwpolicy::regions_launch(atoi(argv[2]), atoll(argv[3]), atoi(argv[4])));
        return 0;
    }
    if (argc != 2) {
        fprintf(stderr, "usage: grid_regions FILE | grid_regions --policy N cells max_regions\n");
        return 2;
    }
    FILE *f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    const double cell_m = rd(f);
    const int gx = ri(f), gz = ri(f), shift = ri(f), calls = ri(f);
    if (!(cell_m > 0.0) || gx < 1 || gz < 1 || (long long)gx * gz > MW_NAV_MAX_CELLS || shift < 0 || shift > 3 || calls < 0) return refused();
    const size_t cells = (size_t)gx * gz;
    std::vector<uint8_t> store(cells + (size_t)shift);
    uint8_t *member = store.data() + shift;
    for (size_t c = 0; c < cells; ++c) {
        const int v = ri(f);
        if (v < 0 || v > 255) short_file();
        member[c] = (uint8_t)v;
    }
    for (int call = 0; call < calls; ++call) {
        const int connectivity = ri(f), min_cells = ri(f), K = ri(f);
        const bool want_sum = ri(f) != 0, want_label = ri(f) != 0;
        if ((connectivity != 4 && connectivity != 8) || min_cells < 1 || K < 1 || K > MW_REGION_MAX) return refused();
        std::vector<uint16_t> label(cells), sizes(cells);
        std::vector<mwregions::Entry> tab((size_t)K);
        std::vector<int32_t> size((size_t)K, -7), cell((size_t)K, -7), sum(want_sum ? (size_t)K * 2 : 0, -7);
        std::vector<int16_t> out(want_label ? cells : 0, -7);
        int rounds = 0;
        const int count = mwregions::regions_one(gx, gz, connectivity, min_cells, K, member, label.data(), sizes.data(), tab.data(), size.data(),
                                                 cell.data(), want_sum ? sum.data() : nullptr, want_label ? out.data() : nullptr, &rounds);
        printf("regions %d %d\n", count, rounds);
        for (int k = 0; k < K; ++k) printf("%d%c", (int)size[(size_t)k], k + 1 == K ? '\n' : ' ');
        for (int k = 0; k < K; ++k) printf("%d%c", (int)cell[(size_t)k], k + 1 == K ? '\n' : ' ');
        if (want_sum)
            for (int k = 0; k < 2 * K; ++k) printf("%d%c", (int)sum[(size_t)k], k + 1 == 2 * K ? '\n' : ' ');
        if (want_label)
            for (size_t c = 0; c < cells; ++c) printf("%d%c", (int)out[c], c + 1 == cells ? '\n' : ' ');
    }
    fclose(f);
    return 0;
}
