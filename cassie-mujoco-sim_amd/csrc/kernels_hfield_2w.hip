/* cassie_hfield.xml, the row-capped fast instantiation in its two-wave form (see kernels_cassie_2w.hip) */
#include "step_kernels.h"
namespace ck {
template void launch_step<32, TopoCassie32, FEAT_HFIELD, FAST_ROWS, 2>(unsigned, hipStream_t, const PhysIO &);
}  // namespace ck
