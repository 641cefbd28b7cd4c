/* cassie_hfield.xml, ALONE (see kernels_cassie_small.hip): the 63-row instantiation, two wavefronts per env, 512 registers a lane */
#include "step_kernels.h"
namespace ck {
template void launch_step<32, TopoCassie32, FEAT_HFIELD, MID_ROWS, 2, false, 1>(unsigned, hipStream_t, const PhysIO &);
}  // namespace ck
