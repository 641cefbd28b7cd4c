/* cassie_tray_box.xml (BASELINE config 5), the fast instantiation (47 rows) in the two-wave form: two wavefronts per env, wave 1
 * running the mass-matrix stage group, the drive-level pass, the factorisations, the bias / passive stage and the stages behind
 * the solve beside wave 0's collision (box-box by the whole wave), velocity, constraint-row and solve stages (physics_kernel.h) */
#include "step_kernels.h"
namespace ck {
template void launch_step<40, TopoCassieTray38, FEAT_WAVEPAIRS, FAST_ROWS_TRAY, 2>(unsigned, hipStream_t, const PhysIO &);
}  // namespace ck
