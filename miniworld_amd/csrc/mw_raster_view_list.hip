// The list forms of the generic-resolution kernels (mw_view_mesh_sub_kernel, mw_view_raster_sub_kernel: same-step auto-reset
// with final observations, mw_engine_frame.hip), compiled in a translation unit of their own: beside the plain kernels, a second
// caller of the shared tile code changed the plain mw_view_raster_kernel's register allocation.
#define MW_VIEW_LIST_UNIT
#include "mw_raster_mesh.hip"
