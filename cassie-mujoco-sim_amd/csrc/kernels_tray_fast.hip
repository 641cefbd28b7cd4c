/* cassie_tray_box.xml (BASELINE config 5), the row-capped instantiation (47 rows) with ONE wavefront per env and 512 registers:
 * the Gram matrix of the staged rows on the matrix core, through the staged tile's own LDS (physics_kernel.h, gram_in_place);
 * a substep with more rows hands the env over to the full instantiation behind it, which walks the hand-over list -- one
 * wavefront per env as well: a workgroup of it fits wherever a workgroup of the fast kernel has retired (the two-wave form of the
 * pass wants two SIMDs with 256 free registers each on one CU, and waited 4 ms for them behind the other env range's one-wave
 * workgroups)
 * (the row-capped instantiation is a LEAN form, pk_stages.h: neither FEAT_READOUT nor FEAT_PROF) */
#include "step_kernels.h"
namespace ck {
template void launch_step<40, TopoCassieTray38, FEAT_WAVEPAIRS, FAST_ROWS_TRAY, 1, false, 1, 0, FEAT_LEAN>(unsigned, hipStream_t, const PhysIO &);
template void launch_step<40, TopoCassieTray38, FEAT_WAVEPAIRS, MID_ROWS, 1, true>(unsigned, hipStream_t, const PhysIO &);
}  // namespace ck
