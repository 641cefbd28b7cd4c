/* the step kernel for cassie_tray_box.xml (BASELINE config 5): 40-dof instantiation (38 used), block-dense factor rows,
 * plane-box / box-box pairs handled by the whole wave; one wave per env, alone, without and with height-field pairs */
#include "step_kernels.h"
namespace ck {
template void launch_step<40, TopoCassieTray38, FEAT_WAVEPAIRS>(unsigned, hipStream_t, const PhysIO &);
template void launch_step<40, TopoCassieTray38, FEAT_ALL>(unsigned, hipStream_t, const PhysIO &);
}  // namespace ck
