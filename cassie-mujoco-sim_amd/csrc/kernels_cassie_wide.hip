/* plain cassie.xml, the 127-row instantiation: two wavefronts per env with 512 registers each, 84 KB of LDS, the solve of a substep
 * with more than 64 rows spread over both (physics_kernel.h, wide_solve).  Alone -- forward / read-out passes, a cassie_sim_t, small
 * batches -- or as the pass that walks the list of envs the 63-row pass handed on. */
#include "step_kernels.h"
namespace ck {
template void launch_step<32, TopoCassie32, 0, WIDE_ROWS, 2, false, 1>(unsigned, hipStream_t, const PhysIO &);
template void launch_step<32, TopoCassie32, 0, WIDE_ROWS, 2, true, 1>(unsigned, hipStream_t, const PhysIO &);
}  // namespace ck
