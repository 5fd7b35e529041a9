// v210_exchange.h -- the cross-lane move of the v210 passes (kernel_interleave.hip unpack_v210_kernel / pack_v210_kernel,
// kernel_widen.hip widen_v210_kernel): device only.  The host programs of tests/host_sanitizer model it by indexing.
#pragma once
#include <hip/hip_runtime.h>

#include "v210_rows.h"

namespace jinc {
namespace v210 {

// The value lane l ^ 1 holds (quad_perm [1, 0, 3, 2]).  Both lanes of a pair are active wherever this is called: pairs of blocks
// start at even blocks and the walk starts at block `lane`.
__device__ __forceinline__ Three from_partner(const Three& t) {
    Three r;
    r.lo = static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(t.lo), 0xB1, 0xF, 0xF, false));
    r.hi = static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(t.hi), 0xB1, 0xF, 0xF, false));
    return r;
}

}  // namespace v210
}  // namespace jinc
