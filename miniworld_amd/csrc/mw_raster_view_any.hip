// The generic-resolution kernels for frames off the 16 x 4 grid and for the wrapper layouts (mw_view_raster_any_kernel and its
// list form), compiled in a translation unit of their own: beside the plain kernels, a second caller of the shared tile code
// changed the plain mw_view_raster_kernel's register allocation.
#define MW_VIEW_LIST_UNIT
#define MW_VIEW_ANY_UNIT
#include "mw_raster_mesh.hip"
