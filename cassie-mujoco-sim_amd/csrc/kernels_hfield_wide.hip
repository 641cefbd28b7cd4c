/* cassie_hfield.xml, the 127-row instantiation (kernels_cassie_wide.hip): what CM_FLAG_HFPRISM's one contact per penetrated grid
 * triangle needs on rough terrain */
#include "step_kernels.h"
namespace ck {
template void launch_step<32, TopoCassie32, FEAT_HFIELD, WIDE_ROWS, 2, false, 1>(unsigned, hipStream_t, const PhysIO &);
template void launch_step<32, TopoCassie32, FEAT_HFIELD, WIDE_ROWS, 2, true, 1>(unsigned, hipStream_t, const PhysIO &);
}  // namespace ck
