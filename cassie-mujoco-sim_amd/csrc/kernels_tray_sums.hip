/* cassie_tray_box.xml: the two-wave fast instantiation (47 rows) WITH the step-sums block (FEAT_SUMS, pk_stages.h) -- what a stepping
 * launch takes while the batch accumulates (kernels_cassie_sums.hip says more).  It keeps FEAT_READOUT like its sibling without the
 * sums, for that sibling's reason (kernels_tray_2w.hip: the register allocator of this 40-dof, 256-register kernel) */
#include "step_kernels.h"
namespace ck {
template void launch_step<40, TopoCassieTray38, FEAT_WAVEPAIRS, FAST_ROWS_TRAY, 2, false, 2, 0, FEAT_READOUT | FEAT_SUMS>(unsigned, hipStream_t, const PhysIO &);
}  // namespace ck
