// Launch-shape constants the kernels and the launch policy (mw_policy.h) share.  Plain preprocessor: no HIP, no types.
#pragma once

#define MW_TILE_W 16
#define MW_TILE_H 4
#define MW_LDS_RECS 32       // triangle records a small-scene raster wave stages in LDS ...
#define MW_LDS_SHADE_Q 7      // ... as the quads K2 reads of each: 7 of the shade record's 8,
#define MW_LDS_CULL_Q 5       //     5 of the classification record's 6 (192 B per triangle: 7.5 KB + 192 B per wave, 5 waves per SIMD)
#define MW_RASTER_REUSE 0x10000     // the raster kernels' flag word: leave clean envs undrawn (mw_kernels.h)
#define MW_STACK_THREADS 256        // the frame stack's copy kernels (mw_stack.hip): lanes, units per lane and chunk
#define MW_STACK_UNROLL 4
