/* cassie_hfield.xml, the row-capped fast instantiation in its two-wave form with the 63-row code behind it in the same kernel
 * (see kernels_cassie_2w_inplace.hip) */
#include "step_kernels.h"
namespace ck {
template void launch_step<32, TopoCassie32, FEAT_HFIELD, FAST_ROWS, 2, false, 2, MID_ROWS>(unsigned, hipStream_t, const PhysIO &);
}  // namespace ck
