/* plain cassie.xml, the row-capped fast instantiation in its two-wave form: two wavefronts per env (128-thread workgroups, two
 * waves per SIMD at 256 registers each), wave 1 running the mass-matrix stage group beside wave 0's collision, velocity and
 * constraint-row stages (physics_kernel.h, env_step) */
#include "step_kernels.h"
namespace ck {
template void launch_step<32, TopoCassie32, 0, FAST_ROWS, 2>(unsigned, hipStream_t, const PhysIO &);
}  // namespace ck
