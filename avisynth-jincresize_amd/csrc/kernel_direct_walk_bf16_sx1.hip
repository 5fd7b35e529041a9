// kernel_direct_walk_bf16_sx1.hip -- see kernel_direct_walk.inc
#define JINC_DIRECT_WALK_T bf16_t
#define JINC_DIRECT_WALK_SX 1
#define JINC_DIRECT_WALK_NAME launch_direct_walk_bf16_sx1
#define JINC_DIRECT_RUNS_NAME launch_direct_runs_bf16_sx1
#include "kernel_direct_walk.inc"
