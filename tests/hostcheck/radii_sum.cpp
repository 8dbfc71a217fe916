// The sums of radii (miniworld_amd/csrc/mw_radii.h) compiled for the host: tests/test_placement_cpu.py evaluates them on the radii
// that the placement fixtures recorded from the reference and compares with the sums the reference formed.
#include "../../miniworld_amd/csrc/mw_radii.h"

extern "C" double mw_radii_sum(double r0, double r1, int f32) { return mw::radii_sum(r0, r1, f32 != 0); }
extern "C" double mw_radii_sum3(double r0, double r1, double more, int f32) { return mw::radii_sum(r0, r1, more, f32 != 0); }
