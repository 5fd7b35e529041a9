// kernel_direct_walk_bf16_sx3.hip -- see kernel_direct_walk.inc
#define JINC_DIRECT_WALK_T bf16_t
#define JINC_DIRECT_WALK_SX 3
#define JINC_DIRECT_WALK_NAME launch_direct_walk_bf16_sx3
#define JINC_DIRECT_RUNS_NAME launch_direct_runs_bf16_sx3
#include "kernel_direct_walk.inc"
