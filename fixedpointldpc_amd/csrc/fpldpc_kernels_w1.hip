// fpldpc_kernels_w1.hip -- the degree-sorted packed table kernel (the W configuration's,
// flood_pk<TableChecks<8, 4, 7, 3>, 4>) and nothing else, in a translation unit of its own so that it
// too gets code-generation options of its own (_build.py SOURCE_FLAGS; the A kernel has
// fpldpc_kernels_a1.hip for the same reason).  The main translation unit (fpldpc_kernels.hip) takes
// the kernel's host stub from here.
#include <hip/hip_runtime.h>

#include "fpldpc_flood_device.hpp"
#include "fpldpc_flood_packed.hpp"
#include "fpldpc_flood_checks_table.hpp"
#include "fpldpc_flood_pk.hpp"

namespace fpldpc {

// (const void *: KArgs lives in each translation unit's unnamed namespace)
const void *table8_pair_kernel() { return reinterpret_cast<const void *>(&flood_pk<TableChecks<8, 4, 7, 3>, 4>); }

}  // namespace fpldpc
