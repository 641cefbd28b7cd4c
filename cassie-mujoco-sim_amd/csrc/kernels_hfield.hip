/* the step kernel for cassie_hfield.xml (BASELINE config 4): 32 dofs, compile-time topology, height-field pairs -- the one-wave
 * forms (see kernels_cassie.hip) */
#include "step_kernels.h"
namespace ck {
template void launch_step<32, TopoCassie32, FEAT_HFIELD>(unsigned, hipStream_t, const PhysIO &);
template void launch_step<32, TopoCassie32, FEAT_HFIELD, FAST_ROWS>(unsigned, hipStream_t, const PhysIO &);
}  // namespace ck
