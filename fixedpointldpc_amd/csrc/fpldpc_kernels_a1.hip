// fpldpc_kernels_a1.hip -- the packed 47-slot array kernel (the A configuration's,
// flood_pk<ArrayChecks<47>, 3>) and nothing else, in a translation unit of its own so that it can be
// compiled with its own code-generation options: the post-RA machine scheduler off (_build.py
// SOURCE_FLAGS), +3.3 % on A at 0 dB and +3.8 % at 4.5 dB, while the other packed kernels lose 1-5 %
// without it (profiles/r5/ab/post_ra.txt).  The main translation unit (fpldpc_kernels.hip) takes the
// kernel's host stub from here, so launches and occupancy queries reach this code object.
#include <hip/hip_runtime.h>

#include "fpldpc_flood_device.hpp"
#include "fpldpc_flood_packed.hpp"
#include "fpldpc_flood_checks_array.hpp"
#include "fpldpc_flood_pk.hpp"

namespace fpldpc {

// (const void *: KArgs lives in each translation unit's unnamed namespace)
const void *array47_pair_kernel() { return reinterpret_cast<const void *>(&flood_pk<ArrayChecks<47>, 3>); }
// the same kernel with the per-output range guard (ArrayChecksOutGuard)
const void *array47_pair_outguard_kernel() { return reinterpret_cast<const void *>(&flood_pk<ArrayChecksOutGuard<47>, 3>); }

}  // namespace fpldpc
