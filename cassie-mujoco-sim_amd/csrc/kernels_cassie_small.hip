/* plain cassie.xml, ALONE -- forward / read-out passes, a single cassie_sim_t, small batches (phys_batch.hip: SMALL_BATCH) -- for
 * models whose caps are 63 rows: the 63-row instantiation with two wavefronts per env AND 512 registers a lane.  A batch that cannot
 * fill the chip has no use for the second workgroup per SIMD pair that the 256-register form makes room for, and at 512 the kernel
 * keeps its row of A in registers (no scratch). */
#include "step_kernels.h"
namespace ck {
template void launch_step<32, TopoCassie32, 0, MID_ROWS, 2, false, 1>(unsigned, hipStream_t, const PhysIO &);
}  // namespace ck
