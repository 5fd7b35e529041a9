// kernel_periodic_launch.h -- the periodic interior kernels are one translation unit per family; this is what crosses between
// them.  launch_periodic (kernel_periodic.hip) alone decides which variant and filter size reach which family; each function
// here picks the instantiations of its own unit for the sample type `io` describes (for_sample_type, kernel_periodic_common.inc)
// and the run-time parameters the router hands it, launches, notes the instance (knobs::note_instance) and returns a hipError_t
// value as int -- hipErrorInvalidValue for parameters its unit has no instance for.  Private to the kernel_periodic*.hip units.
#pragma once
#include "kernels.h"
#include <hip/hip_runtime.h>

namespace jinc {

// kernel_periodic_quad.hip: one period per lane.  fs 7 (ewa_periodic_quad_kernel) and 8 (ewa_periodic_quad8_kernel) on tiles of
// rg = 8 or 4 row groups, fs 9 (ewa_periodic_quad9_kernel) on 4.
int launch_periodic_quad(const PeriodicArgs& pa, const PlaneIO& io, hipStream_t stream, int fs, int rg);
// kernel_periodic_quad2_rg8.hip / _rg4.hip (kernel_periodic_quad2.inc): two periods per lane on the trimmed 6-row support
// (ewa_periodic_quad2_kernel), tiles of 8 / 4 row groups; compute the border columns of pa.edge.
int launch_periodic_quad2_rg8(const PeriodicArgs& pa, const PlaneIO& io, hipStream_t stream);
int launch_periodic_quad2_rg4(const PeriodicArgs& pa, const PlaneIO& io, hipStream_t stream);
// kernel_periodic_quad2x8.hip: two periods per lane on the trimmed 8-row support (ewa_periodic_quad2x8_kernel), tiles of 4 row
// groups; computes the border columns of pa.edge.
int launch_periodic_quad2x8(const PeriodicArgs& pa, const PlaneIO& io, hipStream_t stream);
// kernel_periodic_rows.hip: the row-streamed kernel (ewa_periodic_rows_kernel), fs 3 .. 17.
int launch_periodic_rows(const PeriodicArgs& pa, const PlaneIO& io, hipStream_t stream, int fs);

}  // namespace jinc
