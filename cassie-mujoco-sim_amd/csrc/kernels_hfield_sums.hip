/* cassie_hfield.xml: the two-wave fast instantiation WITH the step-sums block (FEAT_SUMS, pk_stages.h) -- what a stepping launch takes
 * while the batch accumulates (kernels_cassie_sums.hip says more) */
#include "step_kernels.h"
namespace ck {
template void launch_step<32, TopoCassie32, FEAT_HFIELD, FAST_ROWS, 2, false, 2, 0, FEAT_SUMS>(unsigned, hipStream_t, const PhysIO &);
}  // namespace ck
