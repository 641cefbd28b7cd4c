/* plain cassie.xml, the row-capped fast instantiation in its two-wave form: two wavefronts per env (128-thread workgroups, two
 * waves per SIMD at 256 registers each), wave 1 running the mass-matrix stage group beside wave 0's collision, velocity and
 * constraint-row stages (physics_kernel.h, env_step)
 * (a LEAN form, pk_stages.h: neither FEAT_READOUT nor FEAT_PROF -- the launcher never starts it with the read-out block, as a
 * forward pass or with the stage stamps on, step_policy.h) */
#include "step_kernels.h"
namespace ck {
template void launch_step<32, TopoCassie32, 0, FAST_ROWS, 2, false, 2, 0, FEAT_LEAN>(unsigned, hipStream_t, const PhysIO &);
}  // namespace ck
