/* the step kernel for any other model of the supported MJCF subset (dof tree read from the model at run time), and the
 * all-features instantiation of the Cassie topology (a Cassie model with both height-field and box pairs) */
#include "step_kernels.h"
namespace ck {
template void launch_step<32, TopoCassie32, FEAT_ALL>(unsigned, hipStream_t, const PhysIO &);
template void launch_step<32, TopoRuntime, FEAT_ALL>(unsigned, hipStream_t, const PhysIO &);
template void launch_step<40, TopoRuntime, FEAT_ALL>(unsigned, hipStream_t, const PhysIO &);
}  // namespace ck
