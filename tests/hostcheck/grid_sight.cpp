// The host path of miniworld_amd/csrc/mw_sight.h, as a program of its own (tests/test_sight_cpu.py builds it with the address and
// undefined-behaviour sanitizers): one env's grids and viewpoints from a file, the gains and the seen plane of mwsight::sight_one.
//
// The file (hostcheck.h: the tokens):
//   cell range cos_half gx gz shift views has_weight has_dirs agent
//   with agent != 0: min_x max_x min_z max_z, then agent_x agent_z agent_dir (views = 1, no cells, no dirs)
//   gz * gx bytes of opaque, then of weight where the file has them, then of seen as it stands before the call
//   without agent: views cells, then views dirs where the file has them
// `shift` (0 .. 3) is the distance of every byte row from a 4-byte boundary, and each row is the last bytes of an allocation of its own,
// so that the sanitizer sees a read past either end (nav_grid.cpp's rows).  The cell, dir and gain rows hold exactly `views` entries.
// The answer: "sight <covered>", the views gains, the gz * gx bytes of seen.
//
// `grid_sight --matrix FILE` reads the same file and prints, for every cell A of the grid as the viewpoint (heading 0), a row of gx * gz
// digits: 1 where A sees B under the file's range and cone; `grid_sight --policy N cells weighted views` prints mwpolicy::sight_launch:
// "grid threads lds fits"; `grid_sight --reach cell range limit` prints mwsight::reach_cells.
#define HOSTCHECK_PROGRAM "grid_sight"
#include "hostcheck.h"

#include <string>

#include "../../miniworld_amd/csrc/mw_policy.h"
#include "../../miniworld_amd/csrc/mw_sight.h"

using namespace hostcheck;

namespace {

// a row of `cells` bytes that starts `shift` bytes behind a 4-byte boundary and ends with its allocation
struct Row {
    std::vector<uint8_t> store;
    uint8_t *at = nullptr;
    Row(size_t cells, int shift) : store(cells + (size_t)shift), at(store.data() + shift) {}
    void read(FILE *f, size_t cells)
    {
        for (size_t c = 0; c < cells; ++c) {
            const int v = ri(f);
            if (v < 0 || v > 255) short_file();
            at[c] = (uint8_t)v;
        }
    }
};

}  // namespace

int main(int argc, char **argv)
{
    if (argc == 6 && !strcmp(argv[1], "--policy")) {
        print_launch(mwpolicy::sight_launch(atoi(argv[2]), atoll(argv[3]), atoi(argv[4]) != 0, atoi(argv[5])));
        return 0;
    }
    if (argc == 5 && !strcmp(argv[1], "--reach")) {
        printf("%d\n", mwsight::reach_cells(atof(argv[2]), atof(argv[3]), atoi(argv[4])));
        return 0;
    }
    const bool matrix = argc == 3 && !strcmp(argv[1], "--matrix");
    if (argc != 2 && !matrix) {
        fprintf(stderr, "usage: grid_sight [--matrix] FILE | grid_sight --policy N cells weighted views | grid_sight --reach cell range limit\n");
        return 2;
    }
    FILE *f = fopen(argv[argc - 1], "r");
    if (!f) { perror(argv[argc - 1]); return 2; }
    mw_nav_params p{};
    p.cell = rd(f);
    mwseen::Sight s{0.0, 0.0, 0};
    s.range = rd(f); s.cos_half = rd(f);
    p.gx = ri(f); p.gz = ri(f);
    const int shift = ri(f), views = ri(f);
    const bool has_weight = ri(f) != 0, has_dirs = ri(f) != 0, agent = ri(f) != 0;
    if (!(p.cell > 0.0) || p.gx < 1 || p.gz < 1 || (long long)p.gx * p.gz > MW_NAV_MAX_CELLS || shift < 0 || shift > 3 || !(s.range > 0.0) ||
        !(s.range < INFINITY) || !(s.cos_half >= -1.0 && s.cos_half <= 1.0) || views < 1 || (agent && (views != 1 || has_dirs)) ||
        (!agent && !has_dirs && s.cos_half != -1.0))
        return refused();
    World w;
    if (agent) {
        w.read(f, EXTENT);
        w.read(f, POSE);
    }
    const size_t cells = (size_t)p.gx * p.gz;
    Row opaque(cells, shift), weight(has_weight ? cells : 0, shift), seen(cells, shift);
    opaque.read(f, cells);
    if (has_weight) weight.read(f, cells);
    seen.read(f, cells);
    std::vector<int32_t> eyes(agent ? 0 : (size_t)views);
    for (int32_t &v : eyes) v = ri(f);
    std::vector<double> dirs(has_dirs ? (size_t)views : 0);
    for (double &v : dirs) v = rd(f);
    fclose(f);

    std::vector<uint32_t> bits((cells + 31) / 32);
    const uint8_t *wt = has_weight ? weight.at : nullptr;
    if (matrix) {
        mwsight::zero_bits(bits.data(), (int)cells, 0, 1);
        mwsight::stage_bits(opaque.at, bits.data(), (int)cells, 0, 1, [](uint32_t *word, uint32_t bit) { *word |= bit; });
        std::string line(cells, '0');
        for (size_t a = 0; a < cells; ++a) {
            mwsight::Eye e{(int)a / p.gx, (int)a % p.gx, 0.0, 0.0, true};
            mwsight::heading_of(0.0, s, e.hx, e.hz);
            for (size_t b = 0; b < cells; ++b) line[b] = mwsight::sees(bits.data(), p.gx, p.cell, s, e, (int)b / p.gx, (int)b % p.gx) ? '1' : '0';
            puts(line.c_str());
        }
        return 0;
    }
    std::vector<int32_t> gain((size_t)views);
    const MwRayArgs a = w.ray();
    const bool covered = mwsight::sight_one(a, p, s, 0, views, opaque.at, wt, agent ? nullptr : eyes.data(), has_dirs ? dirs.data() : nullptr, bits.data(),
                                            gain.data(), seen.at);
    printf("sight %d\n", covered ? 1 : 0);
    for (int v = 0; v < views; ++v) printf("%d%c", (int)gain[(size_t)v], v + 1 == views ? '\n' : ' ');
    for (size_t c = 0; c < cells; ++c) printf("%u%c", (unsigned)seen.at[c], c + 1 == cells ? '\n' : ' ');
    return 0;
}
