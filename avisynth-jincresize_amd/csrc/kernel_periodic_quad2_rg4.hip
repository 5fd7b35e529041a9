// kernel_periodic_quad2_rg4.hip -- ewa_periodic_quad2_kernel on tiles of 4 row groups (see kernel_periodic_quad2.inc).
#define JINC_QUAD2_RG 4
#define JINC_QUAD2_LAUNCH launch_periodic_quad2_rg4
#include "kernel_periodic_quad2.inc"
