// The reference's sums of radii as they evaluate under NumPy 2's promotion rules (the fixtures record the version: meta/numpy).
// A MeshEnt's radius (Ball, Key, MedKit, the static meshes) comes from ObjMesh.max_coords and is an np.float32 (entity.py:141-147);
// a Box's, a frame's and the agent's are Python floats.  Where a Python float meets an np.float32 it is converted to float32
// first, and the sum is formed in float32, left to right as the reference writes it; the comparison with the float64 distance
// (or the product with the float64 direction vector) widens the result again.  `f32` is decided by the entities' kind (a mesh
// takes part), never by whether a value happens to be representable.
// One statement for the step kernels (mw_setup_common.h), the device generators' placement tests (mw_gen.h) and the host check
// (tests/hostcheck/radii_sum.cpp).
#pragma once
#include "mw_hd.h"

namespace mw {

MW_HD double radii_sum(double r0, double r1, bool f32) { return f32 ? (double)((float)r0 + (float)r1) : r0 + r1; }
MW_HD double radii_sum(double r0, double r1, double more, bool f32)
{
    return f32 ? (double)(((float)r0 + (float)r1) + (float)more) : r0 + r1 + more;
}

}   // namespace mw
