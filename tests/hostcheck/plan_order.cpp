// The ordered frame plan's host-and-device functions (miniworld_amd/csrc/mw_frame_plan.h: the cost class of an env, the class counts
// of the head, the slot lookup of the quad kernel's workgroups) and the policy helper that bounds it (mw_policy.h:
// frame_plan_ordered), as a stand-alone host program: tests/test_plan_order_cpu.py compiles it with the address and
// undefined-behaviour sanitizers and compares its answers with a model in Python.  One query per line of standard input, one answer
// per line of output:
//   C n <n lengths>          the cost class of each display-list length
//   O N                      frame_plan_ordered(N), MW_PLAN_WORDS(N, that), MW_PLAN_COPY(N) and MW_PLAN_DRAW(N, c) for every class
//   L N n_copy c0 .. c7      a block of exactly MW_PLAN_WORDS(N, true) words on the heap, its head filled as the plan kernel fills it
//                            (the counts packed 16 bits each) and every place of every list marked with its own address; then,
//                            as the quad kernel's prologue does for workgroup b = 0 .. N - 1: the counts unpacked from the head, the
//                            lookup, and the word the workgroup would load.  Answers per b: 1 class rank word (draws), 2 0 index
//                            word (copies), 3 0 index 0 (leaves)
#include <cstdio>
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
        if (what == "C") {
            size_t n; in >> n;
            std::string out;
            for (size_t i = 0; i < n; ++i) { long long v; in >> v; out += std::to_string(mw_plan_cost_class((int32_t)v)) + " "; }
            if (!in) { std::puts("bad query"); return 2; }
            std::puts(out.c_str());
        } else if (what == "O") {
            long long N; in >> N;
            if (!in) { std::puts("bad query"); return 2; }
            const bool ord = mwpolicy::frame_plan_ordered((int)N);
            std::printf("%d %zu %zu", ord ? 1 : 0, (size_t)MW_PLAN_WORDS(N, ord), (size_t)MW_PLAN_COPY(N));
            for (int c = 0; c < MW_PLAN_CLASSES; ++c) std::printf(" %zu", (size_t)MW_PLAN_DRAW(N, c));
            std::puts("");
        } else if (what == "L") {
            long long N; uint32_t n_copy, cnt[MW_PLAN_CLASSES];
            in >> N >> n_copy;
            for (uint32_t &c : cnt) in >> c;
            if (!in || N < 1) { std::puts("bad query"); return 2; }
            std::vector<uint32_t> block(MW_PLAN_WORDS(N, true));
            for (size_t i = MW_PLAN_HEAD; i < block.size(); ++i) block[i] = (uint32_t)i;
            uint64_t lo = 0, hi = 0;
            uint32_t n_draw = 0;
            for (uint32_t c = 0; c < MW_PLAN_CLASSES; ++c) { (c < 4 ? lo : hi) += (uint64_t)cnt[c] << (16 * (c & 3)); n_draw += cnt[c]; }
            block[0] = n_draw; block[1] = n_copy; block[2] = MW_PLAN_CLASSES;
            block[MW_PLAN_CLS_LO] = (uint32_t)lo; block[MW_PLAN_CLS_LO + 1] = (uint32_t)(lo >> 32);
            block[MW_PLAN_CLS_HI] = (uint32_t)hi; block[MW_PLAN_CLS_HI + 1] = (uint32_t)(hi >> 32);
            std::string out;
            for (uint32_t b = 0; b < (uint32_t)N; ++b) {
                const uint32_t *plan = block.data();
                const uint64_t c_lo = plan[MW_PLAN_CLS_LO] | (uint64_t)plan[MW_PLAN_CLS_LO + 1] << 32, c_hi = plan[MW_PLAN_CLS_HI] | (uint64_t)plan[MW_PLAN_CLS_HI + 1] << 32;
                uint32_t count[MW_PLAN_CLASSES], cls = 99, rank = 0;
                for (uint32_t c = 0; c < MW_PLAN_CLASSES; ++c) count[c] = mw_plan_class_count(c_lo, c_hi, c);
                const bool draws = mw_plan_slot(b, count, &cls, &rank);
                uint32_t kind, word = 0;
                if (draws) {
                    kind = 1;
                    if (rank >= (uint32_t)N) { std::puts("rank past the segment"); return 3; }
                    word = block.at(MW_PLAN_DRAW(N, cls) + rank);
                } else if (rank < plan[1]) { kind = 2; word = block.at(MW_PLAN_COPY(N) + rank); }
                else kind = 3;
                out += std::to_string(kind) + " " + std::to_string(cls) + " " + std::to_string(rank) + " " + std::to_string(word) + " ";
            }
            std::puts(out.c_str());
        } else { std::puts("bad query"); return 2; }
    }
    return 0;
}
