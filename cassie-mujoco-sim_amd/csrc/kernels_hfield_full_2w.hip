/* cassie_hfield.xml, the 63-row instantiation in its two-wave form as the pass behind the two-wave fast kernel (kernels_cassie_full_2w.hip) */
#include "step_kernels.h"
namespace ck {
template void launch_step<32, TopoCassie32, FEAT_HFIELD, MID_ROWS, 2, true>(unsigned, hipStream_t, const PhysIO &);
}  // namespace ck
