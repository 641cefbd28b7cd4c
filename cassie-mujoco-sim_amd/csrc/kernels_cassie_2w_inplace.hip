/* plain cassie.xml, the row-capped fast instantiation in its two-wave form WITH the 63-row code behind it in the same kernel
 * (cassie_step_kernel's INROWS, round 6): a substep that needs more than 31 rows is finished in place by the 63-row instantiation's
 * code and the env returns to the fast code -- no hand-over list, no pass behind the kernel for models whose caps are 63 rows
 * (a LEAN form, pk_stages.h: neither FEAT_READOUT nor FEAT_PROF -- the launcher never starts it with the read-out block, as a
 * forward pass or with the stage stamps on, step_policy.h) */
#include "step_kernels.h"
namespace ck {
template void launch_step<32, TopoCassie32, 0, FAST_ROWS, 2, false, 2, MID_ROWS, FEAT_LEAN>(unsigned, hipStream_t, const PhysIO &);
}  // namespace ck
