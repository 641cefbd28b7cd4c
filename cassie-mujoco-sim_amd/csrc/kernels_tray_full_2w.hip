/* cassie_tray_box.xml, the full instantiation (63 rows) in the two-wave form: alone, or as the list-walking pass behind the fast one */
#include "step_kernels.h"
namespace ck {
template void launch_step<40, TopoCassieTray38, FEAT_WAVEPAIRS, MID_ROWS, 2>(unsigned, hipStream_t, const PhysIO &);
template void launch_step<40, TopoCassieTray38, FEAT_WAVEPAIRS, MID_ROWS, 2, true>(unsigned, hipStream_t, const PhysIO &);
}  // namespace ck
