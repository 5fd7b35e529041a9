// kernel_periodic_quad2_rg8.hip -- ewa_periodic_quad2_kernel on tiles of 8 row groups (see kernel_periodic_quad2.inc).
#define JINC_QUAD2_RG 8
#define JINC_QUAD2_LAUNCH launch_periodic_quad2_rg8
#include "kernel_periodic_quad2.inc"
