/* cassie_hfield.xml, the row-capped fast instantiation in its two-wave form with the 63-row code behind it in the same kernel
 * (see kernels_cassie_2w_inplace.hip)
 * (a LEAN form, pk_stages.h: neither FEAT_READOUT nor FEAT_PROF -- the launcher never starts it with the read-out block, as a
 * forward pass or with the stage stamps on, step_policy.h) */
#include "step_kernels.h"
namespace ck {
template void launch_step<32, TopoCassie32, FEAT_HFIELD, FAST_ROWS, 2, false, 2, MID_ROWS, FEAT_LEAN>(unsigned, hipStream_t, const PhysIO &);
}  // namespace ck
