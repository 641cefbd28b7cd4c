/* the step kernel for cassie_hfield.xml (BASELINE config 4): 32 dofs, compile-time topology, height-field pairs -- the one-wave
 * forms (see kernels_cassie.hip)
 * (the one-wave fast kernel is a LEAN form, pk_stages.h: neither FEAT_READOUT nor FEAT_PROF) */
#include "step_kernels.h"
namespace ck {
template void launch_step<32, TopoCassie32, FEAT_HFIELD>(unsigned, hipStream_t, const PhysIO &);
template void launch_step<32, TopoCassie32, FEAT_HFIELD, FAST_ROWS, 1, false, 1, 0, FEAT_LEAN>(unsigned, hipStream_t, const PhysIO &);
}  // namespace ck
