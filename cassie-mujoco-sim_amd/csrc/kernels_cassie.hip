/* the step kernel for plain cassie.xml (BASELINE configs 1-3): 32 dofs, compile-time topology, no height-field / box code --
 * the one-wave forms: alone (a large grid: forward / read-out passes of a whole batch, the fast kernel switched off) or as the
 * pass behind the one-wave fast kernel that looks every env's record up, and the one-wave fast kernel
 * (the one-wave fast kernel is a LEAN form, pk_stages.h: neither FEAT_READOUT nor FEAT_PROF) */
#include "step_kernels.h"
namespace ck {
template void launch_step<32, TopoCassie32, 0>(unsigned, hipStream_t, const PhysIO &);
template void launch_step<32, TopoCassie32, 0, FAST_ROWS, 1, false, 1, 0, FEAT_LEAN>(unsigned, hipStream_t, const PhysIO &);
}  // namespace ck
