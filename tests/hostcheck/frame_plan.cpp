// The frame plan's decision (miniworld_amd/csrc/mw_frame_plan.h) and the policy helper that says when a plan is made (mw_policy.h:
// frame_plans), as a stand-alone host program: tests/test_frame_plan_cpu.py compiles it with the address and undefined-behaviour
// sanitizers and compares its answers with a model in Python.  One query per line of standard input, one answer per line of output:
//   V clean reuse slots n <n hex words>   the verdict for one env; the words: the key (MW_FC_KEY_WORDS), then the env's row of the key
//                                         table (MW_FC_META_WORDS(slots); none with slots = 0: no cache).  Answers both forms of the
//                                         decision — from the tables, and from the match mask as the plan kernel's lanes build it
//   P reuse source cache hold path listed N     frame_plans over a FramePolicy
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../miniworld_amd/csrc/mw_frame_plan.h"
#include "../../miniworld_amd/csrc/mw_policy.h"

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        if (!(in >> what)) continue;
        if (what == "V") {
            int clean, reuse, slots; size_t n;
            in >> clean >> reuse >> slots >> n;
            // (exactly the words of the query, on the heap: a read past the key or the row is the sanitizer's to report)
            std::vector<uint64_t> key(MW_FC_KEY_WORDS), meta(n - MW_FC_KEY_WORDS);
            in >> std::hex;
            for (uint64_t &w : key) in >> w;
            for (uint64_t &w : meta) in >> w;
            if (!in || meta.size() != (slots ? (size_t)MW_FC_META_WORDS(slots) : 0u)) { std::puts("bad query"); return 2; }
            const uint32_t whole = mw_frame_verdict_of(clean != 0, reuse != 0, key.data(), slots ? meta.data() : nullptr, slots);
            uint32_t match = 0u;
            for (int j = 0; j < slots; ++j) match |= mw_fc_key_equal(meta.data() + 2 + MW_FC_KEY_WORDS * j, key.data()) ? 1u << j : 0u;
            // (the lanes of the slots the cache does not have report no match; the bits above them must not count either)
            const uint32_t lanes = mw_frame_verdict(clean != 0, reuse != 0, match | 0xFFFFFF00u, slots ? (uint32_t)meta[0] : 0u, slots);
            std::printf("%u %u %u %u\n", whole & 0xFFu, whole >> 8, lanes & 0xFFu, lanes >> 8);
        } else if (what == "P") {
            int reuse, source, cache, hold, path, listed; long long N;
            in >> reuse >> source >> cache >> hold >> path >> listed >> N;
            if (!in) { std::puts("bad query"); return 2; }
            const mwpolicy::FramePolicy pol{reuse != 0, source != 0, cache != 0, hold != 0};
            std::printf("%d\n", mwpolicy::frame_plans(pol, path, listed != 0, (int)N) ? 1 : 0);
        } else { std::puts("bad query"); return 2; }
    }
    return 0;
}
