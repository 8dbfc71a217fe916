// The dealing rule of the small-scene geometry kernel (miniworld_amd/csrc/mw_geom_deal.h) and the policy helper that switches it on
// (mw_policy.h: geom_deals), as a stand-alone host program: tests/test_geom_deal_cpu.py compiles it with the address and
// undefined-behaviour sanitizers and checks its answers.  One query per line of standard input, one answer per line of output:
//   D L n mask     a group of n <= 64 envs served at L lanes per env, mask in hex: as the kernel does, the wavefronts that serve the
//                  group — min(L, ceil(n / (64 / L))) — and for every wavefront i and slot j < 64 / L the env mw_geom_deal names, -1
//                  for an empty slot.  Answer: waves, then waves x (64 / L) numbers, wavefront by wavefront
//   S mask r       mw_deal_select: the position of the set bit of rank r, -1 where there is none
//   P plans enabled lanes    geom_deals
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "../../miniworld_amd/csrc/mw_geom_deal.h"
#include "../../miniworld_amd/csrc/mw_policy.h"

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        if (!(in >> what)) continue;
        if (what == "D") {
            int L, n; uint64_t mask;
            in >> L >> n >> std::hex >> mask;
            if (!in || (L != 8 && L != 16 && L != 32) || n < 1 || n > 64) { std::puts("bad query"); return 2; }
            const int epw = 64 / L, need = (n + epw - 1) / epw, waves = need < L ? need : L;
            std::string out = std::to_string(waves);
            for (int i = 0; i < waves; ++i)
                for (int j = 0; j < epw; ++j) out += " " + std::to_string(mw_geom_deal(mask, waves, i, j));
            std::puts(out.c_str());
        } else if (what == "S") {
            uint64_t mask; int r;
            in >> std::hex >> mask >> std::dec >> r;
            if (!in) { std::puts("bad query"); return 2; }
            std::printf("%d\n", mw_deal_select(mask, r));
        } else if (what == "P") {
            int plans, enabled, lanes;
            in >> plans >> enabled >> lanes;
            if (!in) { std::puts("bad query"); return 2; }
            std::printf("%d\n", mwpolicy::geom_deals(plans != 0, enabled != 0, lanes) ? 1 : 0);
        } else { std::puts("bad query"); return 2; }
    }
    return 0;
}
