// The quad kernel's binning arithmetic (miniworld_amd/csrc/mw_quad_bin.h: the edge triple's start value at a rectangle, its step, the
// touch / full verdict, the walk over a triangle's bounding tiles) as a stand-alone host program: tests/test_quad_binning_cpu.py
// compiles it with the address and undefined-behaviour sanitizers and compares its answers with the flat formula written in Python.
// The walks are the kernel's: a start value per run of rectangles, one step per rectangle after it.  One query per line of standard
// input, one answer per line of output:
//   W dir W H rw rh run  A0 A1 A2  B0 B1 B2  C0 C1 C2  T0 T1 T2  F0 F1 F2
//        the frame's rw x rh rectangles against one triangle.  dir H: every row of rectangles in runs of `run` rectangles (the last run
//        of a row may be shorter), the start value at a run's first rectangle, a step of rw pixels to the right per rectangle.  dir V:
//        every column from the top, in runs of `run`, a step of rh rows down.  Answer, per rectangle in row-major order: e0 e1 e2 (as
//        signed 32-bit values) and touch | full << 1
//   B bbox tiles_x tiles_y
//        the walk over the box's tiles: ty tx of every tile visited, in order
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../miniworld_amd/csrc/mw_quad_bin.h"

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        if (!(in >> what)) continue;
        if (what == "W") {
            std::string dir;
            long long W, H, rw, rh, run, v[15];
            in >> dir >> W >> H >> rw >> rh >> run;
            for (long long &x : v) in >> x;
            if (!in || (dir != "H" && dir != "V") || W < rw || H < rh || rw < 1 || rh < 1 || run < 1 || W % rw || H % rh) { std::puts("bad query"); return 2; }
            int32_t A[3], B[3], C[3], T[3], F[3];
            for (int k = 0; k < 3; ++k) {
                A[k] = (int32_t)v[k]; B[k] = (int32_t)v[3 + k]; C[k] = (int32_t)(uint32_t)(uint64_t)v[6 + k];
                T[k] = (int32_t)v[9 + k]; F[k] = (int32_t)v[12 + k];
            }
            const int nx = (int)(W / rw), ny = (int)(H / rh);
            std::vector<MwEdge3> val((size_t)nx * ny);
            const bool horiz = dir == "H";
            const MwEdge3 d = horiz ? mw_qb_delta(A, B, (int32_t)rw, 0) : mw_qb_delta(A, B, 0, -(int32_t)rh);
            for (int line_ = 0; line_ < (horiz ? ny : nx); ++line_)
                for (int first = 0; first < (horiz ? nx : ny); first += (int)run) {
                    const int rx = horiz ? first : line_, ry = horiz ? line_ : first;
                    MwEdge3 e = mw_qb_start(A, B, C, rx * (int32_t)rw, (int32_t)(H - rh) - ry * (int32_t)rh);
                    for (int k = 0; k < run && first + k < (horiz ? nx : ny); ++k, mw_qb_step(e, d))
                        val.at((size_t)(horiz ? ry : ry + k) * nx + (horiz ? rx + k : rx)) = e;
                }
            std::string out;
            for (const MwEdge3 &e : val) {
                bool touch, full;
                mw_qb_verdict(e, T, F, touch, full);
                for (int k = 0; k < 3; ++k) out += std::to_string((int32_t)e.e[k]) + " ";
                out += std::to_string((touch ? 1 : 0) | (full ? 2 : 0)) + " ";
            }
            std::puts(out.c_str());
        } else if (what == "B") {
            unsigned long long bbox; long long tiles_x, tiles_y;
            in >> bbox >> tiles_x >> tiles_y;
            if (!in || tiles_x < 1 || tiles_y < 1) { std::puts("bad query"); return 2; }
            const MwTileBox box = mw_qb_box((uint32_t)bbox, (int32_t)tiles_x, (int32_t)tiles_y);
            std::string out;
            for (int ty = 0; ty < tiles_y; ++ty) {
                if (!mw_qb_box_row(box, ty)) continue;
                for (int tx = box.x0; tx <= box.x1; ++tx) out += std::to_string(ty) + " " + std::to_string(tx) + " ";
            }
            std::puts(out.c_str());
        } else { std::puts("bad query"); return 2; }
    }
    return 0;
}
