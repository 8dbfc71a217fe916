// MW_HD: a function the HIP kernels call and the host tests compile with a plain C++ compiler (tests/hostcheck/mwhost.cpp).
#pragma once

#ifdef __HIPCC__
#define MW_HD __host__ __device__ inline
#else
#define MW_HD inline
#endif
